"""CPU-side checks of the output descriptor, include/rmhmc_out.h: the header and the ctypes binding agree (entry points, the
descriptor's fields, its two constants), and the argument checks of the shims and drivers that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from riemannhamiltonianmontecarlo_amd import _capi, experiment, multi_gpu

HEADER = os.path.join(ROOT, "include", "rmhmc_out.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_and_binding_agree():
    syms = set(re.findall(r"\b(rmhmc_[a-z0-9_]+)\s*\(", _header()))
    assert len(syms) == 7, syms
    assert syms == set(_capi.OUT_SIGNATURES), syms ^ set(_capi.OUT_SIGNATURES)
    # one *_sample_to per sampler, and every one of them reachable through Context.sample_to
    assert {name for name, _ in _capi.SAMPLERS_TO.values()} == syms - {"rmhmc_ess_dev"}
    # the new declarations stay out of the ABI the CPU oracle has to export
    assert not syms & set(_capi.SIGNATURES)


def test_descriptor_mirrors_the_header():
    body = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*rmhmc_out\s*;", _header(), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = re.match(r"(int32_t|double)\s+(.*)", decl, flags=re.S).groups()
        for nm in names.split(","):
            nm = nm.strip()
            assert (typ == "double") == nm.startswith("*"), decl   # every double is a pointer, `where` is a value
            fields.append((nm.lstrip("* "), typ))
    assert [f for f, _ in fields] == [f for f, _ in _capi.Out._fields_]
    for (name, typ), (_, ctype) in zip(fields, _capi.Out._fields_):
        assert ctype is (C.c_int32 if typ == "int32_t" else C.c_void_p), name
    assert [f for f, _ in fields] == ["where"] + ["samples"] + list(_capi.SUMMARY_KEYS)
    # C layout: an int32, padding, six pointers
    assert C.sizeof(_capi.Out) == 8 + 6 * C.sizeof(C.c_void_p) and _capi.Out.samples.offset == 8


def test_constants_agree():
    consts = dict(re.findall(r"#define\s+(RMHMC_OUT_[A-Z]+)\s+(\d+)", _header()))
    assert consts == {"RMHMC_OUT_HOST": str(_capi.OUT_HOST), "RMHMC_OUT_DEVICE": str(_capi.OUT_DEVICE)}
    assert _capi.OUT_HOST != _capi.OUT_DEVICE


def test_hip_library_exports_the_new_entry_points(hip):
    assert hip.has_out
    lib = C.CDLL(hip.path)
    for s in _capi.OUT_SIGNATURES:
        assert hasattr(lib, s), s


def test_oracle_is_bound_without_them(oracle):
    assert not oracle.has_out


def test_argument_checks_need_no_gpu():
    X = np.random.RandomState(0).randn(12, 3); t = (X[:, 0] > 0).astype(float)
    with pytest.raises(ValueError, match="batched=True"):
        experiment.run_experiment(X, t, "AMH", n_experiments=2, summary=True, batched=False)
    with pytest.raises(ValueError, match="unknown sampler"):   # before any collective: no process group exists here
        multi_gpu.sample_sharded(X, t, 4, sampler="nope")
    # ... and so is everything else a rank could raise on its own once the collectives have begun
    for kw, msg in ((dict(sampler="HMC", gather="mean"), "gather"), (dict(sampler="HMC", sampler_args={"K": 3}), "sampler_args"),
                    (dict(sampler="AMH", sampler_args={"eps": 1.0}), "sampler_args"), (dict(sampler="Gibbs", theta0=0.0), "theta0"),
                    (dict(sampler="RMHMC", sampler_args={"L": 3}), "sampler_args")):
        with pytest.raises(ValueError, match=msg):
            multi_gpu.sample_sharded(X, t, 4, **kw)
    assert set(_capi.SAMPLER_ARGS) == set(_capi.SAMPLERS_TO)
    for name, fn in experiment.SAMPLERS.items():
        with pytest.raises(ValueError, match="ess_nfft"):
            fn(X, t, ess_nfft="x", verbose=False)
        with pytest.raises(ValueError, match="ess_nfft"):
            fn(X, t, summary=True, ess_nfft="x", verbose=False)
    assert _capi.ess_flags("matlab") == 0 and _capi.ess_flags("python") == _capi.FLAG_ESS_WRAP
    assert set(multi_gpu._SHARDED) == set(experiment.SAMPLERS)
