"""The host checks of a sibling predicate and of the atom-type column (hgx_sibling.hip: atompred_validate,
atom_types_validate; include/hgx_sibling.h) under AddressSanitizer + UBSan, without a GPU:
`make -C hypergraphdb_amd/csrc build/san/sibling_check` links tests/native/sibling_check.cc with the engine's host
code compiled under the sanitizers, and the driver runs as its own executable (the sanitizer runtimes are linked
into it): well-formed programs, every malformed shape, arrays allocated to their exact size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypergraphdb_amd", "csrc")


def test_sibling_validate_under_sanitizers():
    b = subprocess.run(["make", "-C", CSRC, "build/san/sibling_check", "-j8"], capture_output=True, text=True,
                       timeout=1100)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([os.path.join(CSRC, "build", "san", "sibling_check")], capture_output=True, text=True,
                       timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sibling_check: all checks passed" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out
