"""csrc/abi_guard.hpp, the guard every C entry point of api*.hip runs its body through, by its stand-alone check program (plain
and with the host sanitizers): a returned status passes through; a std::runtime_error gives RTK_ERR_INVALID and its message;
std::bad_alloc and `throw 7` give RTK_ERR_INVALID; a set_error that throws still leaves the code; a guarded call inside a
guarded call.  Needs no GPU."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "simd-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "abi_guard_check.cpp")
DEPS = [SRC, os.path.join(PKG, "csrc", "abi_guard.hpp"), os.path.join(ROOT, "include", "rtk.h")]


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
    for line in ("status ok", "std::exception ok", "other exceptions ok", "throwing set_error ok", "nested ok", "all ok"):
        assert line in res.stdout, res.stdout
    return res


def test_abi_guard_status_exceptions_and_nesting():
    """Seven statuses through the guard with the last error untouched; runtime_error, bad_alloc and the standard library's own
    out_of_range as RTK_ERR_INVALID with what(); `throw 7` and a thrown string literal as RTK_ERR_INVALID with one fixed message;
    every one of them again with a set_error that throws (the code, nothing recorded); an inner guarded entry point that
    returns, throws a std::exception or throws 7 under an outer one that returns or throws (abi_guard_check.cpp has the cases)."""
    _run(_build("abi_guard_check", []))


def test_abi_guard_under_host_sanitizers():
    """The same stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once."""
    res = _run(_build("abi_guard_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr and res.stderr == "", res.stderr
