"""The table builder on a machine without a GPU: ie_tables.cpp is a pure host function of (n, q),
so tests/cpp/tables_host.cpp links it alone.  Built with the library's host flags plus the host
address and undefined-behaviour sanitizers (a plain executable, nothing preloaded), it must run
clean and print the cos table the reference's libm gives (tests/golden/cos_table.json -- the
fixture smoke() compares the device copy with)."""
import json
import os
import subprocess

import pytest

from tests import oracle_lib as O

CSRC = os.path.join(O.ROOT, "imageencoder_amd", "csrc")
# HIPFLAGS of the Makefile (the library's host objects), then the sanitizers on the host pass
FLAGS = ["--offload-arch=gfx950", "-mcode-object-version=5", "-O3", "-std=c++17", "-fPIC",
         "-I" + os.path.join(O.ROOT, "include"), "-I" + CSRC, "-ffp-contract=off", "-Wall", "-Wno-unused-function",
         "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = str(tmp_path_factory.mktemp("tables_host") / "tables_host")
    r = subprocess.run([hipcc, *FLAGS, os.path.join(O.ROOT, "tests", "cpp", "tables_host.cpp"),
                        os.path.join(CSRC, "ie_tables.cpp"), "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return out


@pytest.mark.parametrize("name,n", [("matrix.txt", 4), ("matrix8_1.txt", 8)])
def test_cos_table_built_on_the_host(exe, name, n):
    r = subprocess.run([exe, os.path.join(O.GOLDEN, name), str(n)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr  # (a sanitizer report goes to stderr and fails the run)
    got = [float.fromhex(x) for x in r.stdout.split()]
    pinned = [float.fromhex(x) for x in json.load(open(os.path.join(O.GOLDEN, "cos_table.json")))[str(n)]]
    assert got == pinned
