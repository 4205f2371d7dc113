"""What the test modules of the stand-alone host check programs (tests/cpp/*_plan_check.cpp) share: build one with g++ when it is
stale, run it, and look for its lines.  A plain helper module: each test module keeps its own source, dependency list, flags and
expected lines."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def csrc(*names):
    return [os.path.join(PKG, "csrc", n) for n in names]


def stale(exe, deps):
    return not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps)


def build(name, src, deps, flags=(), extra=()):
    """-> tests/cpp/_build/<name>, compiled from src when it is older than any of deps.  flags: the module's own (-ffp-contract=off);
    extra: the sanitizers."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    if stale(exe, deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *flags, "-Wall", "-Wextra", "-Werror", *extra,
                               "-I" + os.path.join(PKG, "csrc"), src, "-o", exe])
    return exe


def run(exe, lines, args=()):
    res = subprocess.run([exe, *args], capture_output=True, text=True)
    assert res.returncode == 0 and "FAILED" not in res.stdout, res.stdout + res.stderr
    for line in lines:
        assert line in res.stdout, res.stdout
    return res


def assert_sanitizers_quiet(res):
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
