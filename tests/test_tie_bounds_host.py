"""The tie limits of build_tables against the reference's FP64 quotient, for every matrix of the
sweep (tests/matrix_sweep.py), without a GPU.  tests/cpp/tie_bounds_host.cpp links ie_tables.cpp
alone, built like tests/test_tables_host.py builds its program: the library's host flags
(-ffp-contract=off among them) plus the host address and undefined-behaviour sanitizers, a plain
executable with nothing preloaded.  The program asserts the bound, the decision and the record
size per coefficient and variant (see its header); this file also compares the FP64-rounded
coefficients it wrote with oracle.quantize on the same blocks, so its restatement of the reference
is tied to the pinned oracle.

Largest |t32 - t64| / bound observed over the sweep (2*10^5 seeded blocks and 1024 tie-frame
blocks per matrix): see DESIGN.md, "The matrix sweep"."""
import os
import subprocess

import numpy as np
import pytest

from tests import matrix_sweep as MS
from tests import oracle_lib as O
from tests.test_tables_host import CSRC, FLAGS

BLOCKS = 200_000
CASES = [(n, name) for n in (4, 8) for name in MS.ids(n)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = str(tmp_path_factory.mktemp("tie_bounds_host") / "tie_bounds_host")
    r = subprocess.run([hipcc, *FLAGS, os.path.join(O.ROOT, "tests", "cpp", "tie_bounds_host.cpp"),
                        os.path.join(CSRC, "ie_tables.cpp"), "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return out


def run_program(exe, tmp_path, n, name, q, blocks=BLOCKS):
    """Runs the program on matrix q; returns (completed process, pixel blocks, coefficients)."""
    mfile, tfile, prefix = tmp_path / f"{name}_{n}.txt", tmp_path / "ties.bin", tmp_path / "out"
    mfile.write_text(" ".join(str(int(v)) for v in q) + "\n")
    ties = MS.to_blocks(MS.tie_frames(n, q, 64 * n, 16 * n, 1, seed=3), n)
    tfile.write_bytes(ties.tobytes())
    r = subprocess.run([exe, str(mfile), str(n), str(blocks), "20261020", str(prefix), str(tfile)],
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return r, None, None
    pix = np.fromfile(str(prefix) + ".pix", dtype=np.uint8).reshape(-1, n * n)
    coef = np.fromfile(str(prefix) + ".coef", dtype=np.int16).reshape(-1, n * n)
    return r, pix, coef


@pytest.mark.parametrize("n,name", CASES, ids=[f"{n}x{n}-{name}" for n, name in CASES])
def test_tie_limits_hold_against_fp64(exe, oracle, tmp_path, n, name):
    q = MS.by_name(n, name)
    r, pix, coef = run_program(exe, tmp_path, n, name, q)
    assert r.returncode == 0 and not r.stderr, r.stderr  # (a sanitizer report goes to stderr and fails the run)
    print(f"{n}x{n} {name}: " + "; ".join(l for l in r.stdout.splitlines() if l.startswith(("ratio", "rec_bits"))))
    out = dict(l.split(" ", 1) for l in r.stdout.splitlines() if l.startswith("blocks"))
    assert int(out["blocks"]) >= BLOCKS
    # the blocks as a frame n pixels wide: block b is rows b*n .. b*n + n - 1
    assert len(pix) == len(coef) >= 3 * 1024 + 1024
    exp = oracle.quantize(pix.reshape(-1, n), n, q)
    bad = np.argwhere(exp != coef)
    assert bad.size == 0, (name, bad[:4].tolist(), pix[bad[0, 0]].tolist())
