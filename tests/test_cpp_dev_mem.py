"""csrc/dev_mem.hpp, the one place the host side of the C-ABI allocates, through its stand-alone check program (plain and with the
host sanitizers): the growth rules, what reserve keeps and re-makes, a failing allocation, moves and swaps, and that nothing is
left allocated at the end.  Needs no GPU: the memory source is a counting malloc."""
import os
import re
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "dev_mem_check.cpp")
DEPS = [SRC, os.path.join(PKG, "csrc", "dev_mem.hpp")]


def _stale(exe, deps):
    return not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps)


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    if _stale(exe, DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                               "-I" + os.path.join(PKG, "csrc"), SRC, "-o", exe])
    return exe


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "FAILED" not in res.stdout, res.stdout + res.stderr
    for line in ("rules ok", "reserve ok", "exactly ok", "failure ok", "moves ok", "vector ok", "masked swap ok", "all ok"):
        assert line in res.stdout, res.stdout
    m = re.search(r"live (\d+) allocs (\d+) frees (\d+)", res.stdout)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) == int(m.group(3)) > 0, res.stdout
    return res


def test_dev_mem_rules_reserve_failure_moves_and_no_leak():
    """Capacities of every rule at 0, 1, 255, 256, 4096 and around the chunk cap; reserve within and beyond capacity; set-exactly
    on a smaller request; a failed allocation and the reserve after it; moves, swaps and a resized vector of owners; the
    make-before-drop of the light table and the masked swap of the geometry sets (dev_mem_check.cpp has the numbers)."""
    _run(_build("dev_mem_check", []))


def test_dev_mem_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = _run(_build("dev_mem_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr and res.stderr == "", res.stderr
