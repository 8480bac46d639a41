"""The host checks of the atoms entry points (include/hgx_atoms.h: the part arrays with the atoms flags, the keep
table, the argument checks that fail before any device work) under AddressSanitizer + UBSan, without a GPU:
`make -C hypergraphdb_amd/csrc build/san/atoms_check` links tests/native/atoms_check.cc with the engine's host code
compiled under the sanitizers, and the driver runs as its own executable (the sanitizer runtimes are linked into
it): well-formed batches, every malformed shape, arrays allocated to their exact size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypergraphdb_amd", "csrc")


def test_atoms_host_checks_under_sanitizers():
    b = subprocess.run(["make", "-C", CSRC, "build/san/atoms_check", "-j8"], capture_output=True, text=True, timeout=1100)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([os.path.join(CSRC, "build", "san", "atoms_check")], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "atoms_check: all checks passed" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out
