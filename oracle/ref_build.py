"""build_ref(): the one place that knows how oracle/_ref/ref_probe_* is made (recipe: ref.mk next to this file).

Imports nothing of the package, so that __graft_entry__.build() can load this file by its path and build from its own tree,
whichever `oracle` package is importable; oracle/__init__.py re-exports the names."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_OUT = os.path.join(_HERE, "_ref")
REF_COMPILER = "/opt/rocm/llvm/bin/clang++"


def reference_dir() -> str:
    """The reference checkout: RTK_REFERENCE_DIR, else the sibling directory `reference` of this repository."""
    return os.environ.get("RTK_REFERENCE_DIR") or os.path.join(os.path.dirname(os.path.dirname(_HERE)), "reference")


def build_ref() -> bool:
    """Compile oracle/_ref/ref_probe_* when the reference and the compiler are here; otherwise do nothing.  -> built or not.
    ref.mk picks the packet widths this host can run."""
    ref = reference_dir()
    if not (os.path.isdir(os.path.join(ref, "include", "raytracer")) and os.path.exists(REF_COMPILER)):
        return False
    subprocess.check_call(["make", "-C", _HERE, "-f", "ref.mk", "-s", f"-j{min(16, os.cpu_count() or 1)}",
                           f"REF={os.path.abspath(ref)}", f"REFCXX={REF_COMPILER}"])
    return True
