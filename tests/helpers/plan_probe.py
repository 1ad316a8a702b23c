"""The shapes csrc/plan.h decides, asked of the compiled rule itself: tests/helpers/plan_probe.cpp built once per process with the host
C++ compiler (plain C++17, no HIP, no GPU) and run as a child process."""
import atexit
import json
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
_exe = None


def probe_exe():
    global _exe
    if _exe is None:
        cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
        assert cxx, "no host C++ compiler"
        tmp = tempfile.mkdtemp(prefix="plan_probe_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        exe = os.path.join(tmp, "plan_probe")
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "plan_probe.cpp")])
        _exe = exe
    return _exe


def probe_line(M, D, n, flags=0, dtype=0, options=(), set_options=()):
    """options / set_options: (key, value) pairs given at create / to rmhmc_set_option afterwards"""
    toks = ["%d %d %d %d %#x" % (M, D, n, dtype, flags)]
    toks += ["%s=%d" % kv for kv in dict(options).items()] + ["set:%s=%d" % kv for kv in dict(set_options).items()]
    return " ".join(toks)


def probe_many(lines):
    """one result dict per input line (probe_line), from one run of the probe"""
    lines = list(lines)
    out = subprocess.run([probe_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines), (len(out), len(lines))
    return [json.loads(o) for o in out]


def probe(M, D, n, flags=0, **kw):
    return probe_many([probe_line(M, D, n, flags, **kw)])[0]


def plan(M, D, n, flags=0, **options):
    """the Plan of an accepted shape, as a dict of its fields"""
    r = probe(M, D, n, flags, options=options)
    assert r["check"]["code"] == 0 and r["option_error"] is None, r
    return r["plan"]
