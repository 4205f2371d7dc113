"""The phase diagnostic (`make phases`, csrc/phases.hip.hpp, tools/phase_times.py) is built by nobody but a person who needs
it: keep it compiling, and keep the tool's column names in step with the header's slot enumeration."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simd-raytracer_amd")


def _makefile_vars():
    """The Makefile's simple assignments, $(NAME) references expanded."""
    out = {}
    for line in open(os.path.join(PKG, "Makefile")):
        m = re.match(r"^(\w+)\s*(?::=|\?=|=)\s*(.*)$", line.rstrip("\n"))
        if m and m.group(1) not in out:
            out[m.group(1)] = re.sub(r"\$\((\w+)\)", lambda r: out.get(r.group(1), ""), m.group(2)).strip()
    return out


def test_diagnostic_flavour_of_the_benchmark_kernel_compiles_without_a_warning(tmp_path):
    mk = _makefile_vars()
    if not os.path.exists(mk["HIPCC"]):
        pytest.skip("no hipcc")
    assert "-Wall" in mk["FLAGS"] and "-DRTK_G4_WAVES=" + mk["G4W"] in mk["FLAGS"], mk["FLAGS"]        # the parser found the real flags
    # (-Wno-unused-command-line-argument: with -S the driver itself warns about the link flag hipcc always adds)
    cmd = [mk["HIPCC"], f"--offload-arch={mk['ARCH']}", *mk["FLAGS"].split(), "-DRTK_DEBUG_PHASES", "-DRTK_ONLY_LEAN_G4",
           "-Wno-unused-command-line-argument", "-S", "--cuda-device-only", "csrc/kernels.hip", "-o", str(tmp_path / "kernels_phases.s")]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr and "warning" not in r.stdout, r.stderr[-4000:]
    assert "k_render" in (tmp_path / "kernels_phases.s").read_text()


def test_tool_and_header_agree_on_the_slots():
    text = open(os.path.join(PKG, "csrc", "phases.hip.hpp")).read()
    body = re.search(r"enum PhaseSlot : int \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    enumerators = [e.split("=")[0].strip() for e in body.split(",") if e.strip()]
    assert enumerators[-1] == "PH_SLOTS" and all(e.startswith("PH_") for e in enumerators), enumerators
    spec = importlib.util.spec_from_file_location("phase_times", os.path.join(ROOT, "tools", "phase_times.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)                       # (loads no library: the tool only measures from main())
    assert tool.SLOTS == [e[len("PH_"):].lower() for e in enumerators[:-1]]
    assert len(tool.SLOTS) == 44 and len(set(tool.SLOTS)) == 44
    # the only explicit value is the first one: every slot's number is its position
    assert re.findall(r"=\s*\w+", body) == ["= 0"]
