#!/usr/bin/env python3
"""Record what the reference computes, as test fixtures: runs the probe (oracle/_ref/ref_probe_*, built by
__graft_entry__.build() from a checkout of the reference) on the inputs of tests/ref_probe_cases.py and writes
tests/golden/ref_probe/<scene>_{queries,frames}.npz (the scene files and the generated variants of tests/material_scenes.py),
the exactly-eps fixture and MANIFEST.json.  The files hold arrays only.  Run again, it writes the same bytes.

    python tools/make_ref_probe_fixtures.py [--check]      (--check: write nothing, fail if a file would change)"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import oracle as ora                      # noqa: E402
import ref_probe_cases as rc              # noqa: E402


def compile_line(width, depth, tree="default"):
    """The recipe's command for a variant, with the reference's place left symbolic."""
    target = os.path.relpath(ora.ref_binary(width, depth, tree), os.path.dirname(ora.REF_OUT))
    out = subprocess.check_output(["make", "-C", os.path.dirname(ora.REF_OUT), "-f", "ref.mk", "-n", "-B", "REF=REFERENCE",
                                   "WIDTHS=4 8 16", target], text=True)
    return [l for l in out.splitlines() if "ref_probe.cpp" in l][0].strip()


def main():
    check = "--check" in sys.argv[1:]
    ora.build()
    need = [(w, 5, "default") for w in rc.WIDTHS] + [(8, 10, "default"), (8, 5, "eps_0.25"), (8, 1, "default"), (8, 16, "default")]
    missing = [ora.ref_binary(*v) for v in need if not ora.ref_available(*v)]
    if missing:
        sys.exit("missing or not runnable on this host (run __graft_entry__.build() with the reference present): " + ", ".join(missing))
    os.makedirs(rc.FIXTURE_DIR, exist_ok=True)
    man = {"what": "arrays written by oracle/ref_probe.cpp, the reference's own code behind a file interface; inputs: tests/ref_probe_cases.py",
           "frame": list(rc.FRAME), "variants": {os.path.basename(ora.ref_binary(*v)): compile_line(*v) for v in need},
           "scenes": {}}
    changed = []
    import material_scenes as ms
    cases = [(name, rel + ".crtscene", lambda name=name, rel=rel: rc.record(ora, ora.load_crtscene(rc.scene_path(rel)), name))
             for name, rel in rc.FIXTURE_SCENES.items()]
    cases += [(name, f"tests/material_scenes.py::make_scene(ora, {v!r})", lambda v=v: rc.record_material(ora, ms.make_scene(ora, v)))
              for name, v in rc.material_fixture_names().items()]
    with tempfile.TemporaryDirectory() as tmp:
        for name, scene, run in cases:
            arrays, argv = run()
            files = {}
            for part in rc.PARTS:
                new = os.path.join(tmp, f"{name}_{part}.npz")
                rc.save_npz(new, {k: v for k, v in arrays.items() if rc.part_of(k) == part})
                data = open(new, "rb").read()
                path = os.path.join(rc.FIXTURE_DIR, f"{name}_{part}.npz")
                if not os.path.exists(path) or open(path, "rb").read() != data:
                    changed.append(path)
                    if not check:
                        open(path, "wb").write(data)
                files[os.path.basename(path)] = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
            man["scenes"][name] = {"scene": scene, "files": files,
                                   "arrays": {k: [str(v.dtype) if v.dtype.names is None else "REF_HIT_DTYPE", list(v.shape)] for k, v in sorted(arrays.items())},
                                   "commands": argv}
            print(name, {k: v["bytes"] for k, v in files.items()})
        from test_random_scenes import _make_scene
        arrays, argv = rc.record_eps(ora, _make_scene(ora, 100))
        new = os.path.join(tmp, rc.EPS_FIXTURE + ".npz")
        rc.save_npz(new, arrays)
        data = open(new, "rb").read()
        path = os.path.join(rc.FIXTURE_DIR, rc.EPS_FIXTURE + ".npz")
        if not os.path.exists(path) or open(path, "rb").read() != data:
            changed.append(path)
            if not check:
                open(path, "wb").write(data)
        man["scenes"][rc.EPS_FIXTURE] = {"scene": "tests/test_random_scenes.py::_make_scene(ora, 100), eps = 0.25",
                                         "files": {os.path.basename(path): {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}},
                                         "arrays": {k: [str(v.dtype) if v.dtype.names is None else "REF_HIT_DTYPE", list(v.shape)] for k, v in sorted(arrays.items())},
                                         "commands": argv}
        print(rc.EPS_FIXTURE, len(data))
    text = json.dumps(man, indent=1, sort_keys=True) + "\n"
    mpath = os.path.join(rc.FIXTURE_DIR, "MANIFEST.json")
    if not os.path.exists(mpath) or open(mpath).read() != text:
        changed.append(mpath)
        if not check:
            open(mpath, "w").write(text)
    if check and changed:
        sys.exit("would change: " + ", ".join(changed))
    print("unchanged" if not changed else "wrote " + ", ".join(os.path.relpath(c, ROOT) for c in changed))


if __name__ == "__main__":
    main()
