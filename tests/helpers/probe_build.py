"""The stand-alone probes of the GPU-free headers (tests/helpers/<name>.cpp), built under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_built = {}


def probe_exe(tmp_path_factory, name):
    """<name>.cpp built with the host compiler under ASan + UBSan; the path of the program, built once per name.  The sanitizers'
    runtime is linked into the program itself, so it starts whatever else the environment preloads; only beside a preloaded library
    that bears the ASan runtime's own name does that runtime refuse to start, and there the default (shared) runtime is the one that
    starts."""
    if name not in _built:
        cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
        assert cxx, "no host C++ compiler"
        tmp = tmp_path_factory.mktemp(name)
        clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        for kind, runtime in (("static", ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]), ("shared", [])):
            exe = str(tmp / (name + "_" + kind))
            subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all"] + runtime + ["-o", exe, os.path.join(_HERE, name + ".cpp")])
            start = subprocess.run([exe], input="", capture_output=True, text=True, timeout=60)   # no input: main returns 2
            if "incompatible ASan runtimes" not in start.stderr:
                break
        assert start.returncode == 2 and not start.stderr, (kind, start.returncode, start.stderr[-2000:])
        _built[name] = exe
    return _built[name]
