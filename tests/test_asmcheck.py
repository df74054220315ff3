"""tools/asmcheck.py (the build's guard that the exact FP64 paths carry no fused multiply-add,
SURVEY Appendix C.4): a correctly rounded division's own Newton steps pass, a contracted a*b+c
scheduled inside a division's window does not."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DIV = """\tv_div_scale_f64 v[16:17], s[22:23], v[12:13], v[12:13], v[10:11]
\tv_rcp_f64_e32 v[38:39], v[16:17]
\tv_div_scale_f64 v[40:41], vcc, v[10:11], v[12:13], v[10:11]
\tv_fma_f64 v[42:43], -v[16:17], v[38:39], 1.0
\tv_fmac_f64_e32 v[38:39], v[38:39], v[42:43]
{inject}\tv_fma_f64 v[42:43], -v[16:17], v[38:39], 1.0
\tv_fmac_f64_e32 v[38:39], v[38:39], v[42:43]
\tv_mul_f64 v[42:43], v[40:41], v[38:39]
\tv_fma_f64 v[16:17], -v[16:17], v[42:43], v[40:41]
\tv_div_fmas_f64 v[16:17], v[16:17], v[38:39], v[42:43]
\tv_div_fixup_f64 v[16:17], v[16:17], v[12:13], v[10:11]
"""


def _run(tmp_path, body):
    p = tmp_path / "k.s"
    p.write_text("_Zkern:\n" + body)
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asmcheck.py"), str(p)],
                          capture_output=True, text=True, timeout=60)


def test_division_steps_pass(tmp_path):
    assert _run(tmp_path, DIV.format(inject="")).returncode == 0


def test_contracted_fma_inside_division_window_fails(tmp_path):
    r = _run(tmp_path, DIV.format(inject="\tv_fma_f64 v[50:51], v[2:3], v[4:5], v[6:7]\n"))
    assert r.returncode == 1 and "v[50:51]" in r.stderr


def test_fma_outside_any_division_fails(tmp_path):
    r = _run(tmp_path, "\tv_fmac_f64_e32 v[2:3], v[4:5], v[6:7]\n" + DIV.format(inject=""))
    assert r.returncode == 1


def _budget_asm(occ, scratch):
    name = "_ZN2ie13encode_kernelILi8ELb0ELb0EEEvNS_7EncArgsEPKNS_9EncTablesE"
    return (f"{name}:\n\ts_endpgm\n; NumVgprs: 121\n; ScratchSize: {scratch}\n; Occupancy: {occ}\n")


def test_register_budget_holds(tmp_path):
    p = tmp_path / "k.s"
    p.write_text(_budget_asm(4, 0))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asmcheck.py"), str(p)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def test_spilling_kernel_over_budget_fails(tmp_path):
    p = tmp_path / "k.s"
    p.write_text(_budget_asm(4, 68))  # the scratch the per-lane pixel rows once cost the 8x8 kernel
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asmcheck.py"), str(p)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "over budget" in r.stderr


def test_built_kernels_within_budget():
    """The in-tree build's assembly (make asm, run by build()) meets the budgets."""
    import glob
    import pytest
    files = sorted(glob.glob(os.path.join(ROOT, "build", "asm", "*.s")))
    if not files:
        pytest.skip("no build/asm (run __graft_entry__.build())")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asmcheck.py")] + files,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_64bit_lds_atomic_fails(tmp_path):
    """A 64-bit LDS atomic in any kernel (the round-5 fault: ds_or_b64 at a 4-byte aligned bit-image
    address raised a memory violation that aborted the queue) fails the build check."""
    r = _run(tmp_path, "\tds_or_b64 v2, v[4:5] offset:8\n\ts_endpgm\n")
    assert r.returncode == 1 and "64-bit LDS atomic" in r.stderr
    r = _run(tmp_path, "\tds_add_rtn_u64 v[6:7], v2, v[4:5]\n")
    assert r.returncode == 1
    assert _run(tmp_path, "\tds_or_b32 v2, v4\n\tds_or_b32 v2, v5 offset:4\n\tds_read_b64 v[4:5], v2\n").returncode == 0


def test_wide_ds_in_inline_asm_fails(tmp_path):
    """Hand-written inline asm may not name a 64/96/128-bit DS instruction (its address alignment is
    beyond the compiler's checks); the 32-bit pair the emission uses passes."""
    good = tmp_path / "good.hip"
    good.write_text('asm volatile("ds_or_b32 %0, %1\\n\\tds_or_b32 %0, %2 offset:4" ::"v"(a), "v"(hi), "v"(lo));\n'
                    "// a comment naming ds_or_b64 is not code\n")
    bad = tmp_path / "bad.hip"
    bad.write_text('asm volatile("ds_or_b64 %0, %1" ::"v"(a), "v"(x));\n')
    tool = os.path.join(ROOT, "tools", "asmcheck.py")
    assert subprocess.run([sys.executable, tool, str(good)], capture_output=True, text=True).returncode == 0
    r = subprocess.run([sys.executable, tool, str(bad)], capture_output=True, text=True)
    assert r.returncode == 1 and "bad.hip:1" in r.stderr


def test_sources_have_no_wide_inline_ds():
    import glob
    srcs = [f for ext in ("hip", "h", "hpp") for f in glob.glob(os.path.join(ROOT, "imageencoder_amd", "csrc", f"*.{ext}"))]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asmcheck.py")] + srcs,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
