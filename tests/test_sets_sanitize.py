"""The host checks of the visited-sets readout (hgx_sets.hip: sets_validate; the argument checks of
include/hgx_sets.h) under AddressSanitizer + UBSan, without a GPU: `make -C hypergraphdb_amd/csrc
build/san/sets_check` links tests/native/sets_check.cc with the engine's host code compiled under the sanitizers,
and the driver runs as its own executable (the sanitizer runtimes are linked into it): well-formed selections, every
refusal that needs no device, arrays allocated to their exact size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypergraphdb_amd", "csrc")


def test_sets_validate_under_sanitizers():
    b = subprocess.run(["make", "-C", CSRC, "build/san/sets_check", "-j8"], capture_output=True, text=True,
                       timeout=1100)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([os.path.join(CSRC, "build", "san", "sets_check")], capture_output=True, text=True,
                       timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sets_check: all checks passed" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out
