#!/usr/bin/env python3
"""Compare the functions of two sets of `--cuda-device-only -S` assembly files: is the generated
code the same?  For a refactor that may not change one instruction.

    python3 tools/isa_diff.py --old OLD.s [...] --new NEW.s [...] [--rename REGEX REPL]

Functions are matched by symbol name (--rename rewrites the OLD names first, e.g. for a dropped
template argument).  Per function the instruction stream is compared line by line after stripping
comments, directive lines, the numbers of compiler labels and symbol names; for kernels the
.amdhsa_* descriptor and the register / scratch / LDS / kernarg / workgroup-size metadata must be
equal too.  Prints one line per function; exit status 1 on any difference or unmatched function.

--mask-kernarg, for a change that only removes or adds members of a kernel-argument struct, masks
exactly two things: the immediate offset of scalar loads whose base is the kernel-argument pointer
(the user SGPR pair the kernel's descriptor assigns to it; registers and widths still compare), and
the kernarg-size lines (.amdhsa_kernarg_size in the descriptor, kernarg_segment_size in the
metadata).
"""
import argparse
import difflib
import re
import sys

META = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "kernarg_segment_size", "max_flat_workgroup_size")


def parse(path):
    """{symbol: {"code": [normalised lines], "desc": [.amdhsa_* lines], "meta": {key: value}}}"""
    funcs, cur, desc = {}, None, None
    text = open(path).read()
    for ln in text.split("\n"):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = funcs.setdefault(m.group(1), {"code": [], "desc": [], "meta": {}})
            continue
        s = ln.split(";", 1)[0].strip()
        if not s:
            continue
        if s.startswith(".amdhsa_kernel"):
            desc = funcs[s.split()[1]]["desc"]
        elif s.startswith(".end_amdhsa_kernel"):
            desc = None
        elif desc is not None:
            desc.append(" ".join(s.split()))
        if re.match(r"^\.Lfunc_end\d+:", s):
            cur = None
        if cur is None:
            continue
        if re.match(r"^\.LBB\d+_\d+:", s):
            cur["code"].append(".LBB:")
        elif not s.startswith("."):
            s = re.sub(r"\.LBB\d+_\d+", ".LBB", s)
            s = re.sub(r"\.L__unnamed_\d+", ".Lunnamed", s)
            cur["code"].append(" ".join(re.sub(r"_Z\w+(\.const)?", "SYM", s).split()))
    k = text.find("amdhsa.kernels")
    for ent in text[k:].split("\n  - ")[1:] if k >= 0 else []:
        m = re.search(r"\.name:\s+(\S+)", ent)
        if m and m.group(1) in funcs:
            for key in META:
                v = re.search(rf"\.{key}:\s+(\d+)", ent)
                funcs[m.group(1)]["meta"][key] = int(v.group(1)) if v else None
    return {n: f for n, f in funcs.items() if f["code"]}  # (data symbols have no instructions)


def mask_kernarg(f):
    """Drop what moves when the kernel-argument struct changes size (kernels only)."""
    if not f["desc"]:
        return
    user = {m.group(1): int(m.group(2)) for m in (re.match(r"\.amdhsa_user_sgpr_(\w+) (\d+)$", d) for d in f["desc"]) if m}
    # user SGPRs are assigned in this order: the kernarg pointer follows the enabled ones before it
    lo = 4 * user.get("private_segment_buffer", 0) + 2 * user.get("dispatch_ptr", 0) + 2 * user.get("queue_ptr", 0)
    load = re.compile(rf"^(s_load_\w+ \S+ s\[{lo}:{lo + 1}\],) (?:0x[0-9a-f]+|\d+)\b")
    if user.get("kernarg_segment_ptr"):
        f["code"] = [load.sub(r"\1 KERNARG_OFFSET", c) for c in f["code"]]
    f["desc"] = [d for d in f["desc"] if not d.startswith(".amdhsa_kernarg_size ")]
    f["kernarg"] = f["meta"].pop("kernarg_segment_size", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--rename", nargs=2, metavar=("REGEX", "REPL"))
    ap.add_argument("--mask-kernarg", action="store_true",
                    help="ignore kernel-argument load offsets and the kernarg size (a struct member removed)")
    ap.add_argument("-v", action="store_true", help="print the first differing lines")
    a = ap.parse_args()
    old, new = {}, {}
    for p in a.old:
        for n, f in parse(p).items():
            old[re.sub(a.rename[0], a.rename[1], n) if a.rename else n] = f
    for p in a.new:
        new.update(parse(p))
    if a.mask_kernarg:
        for f in list(old.values()) + list(new.values()):
            mask_kernarg(f)
    rc = 0
    for n in sorted(set(old) | set(new)):
        if n not in old or n not in new:
            print(f"{n}: only in {'old' if n in old else 'new'}")
            rc = 1
            continue
        o, w = old[n], new[n]
        same = o["code"] == w["code"] and o["desc"] == w["desc"] and o["meta"] == w["meta"]
        res = " ".join(f"{k}={v}" for k, v in w["meta"].items() if v is not None)
        if w.get("kernarg") is not None:  # (masked: shown, not compared)
            res += f" kernarg_segment_size={o.get('kernarg')}->{w['kernarg']}"
        print(f"{n}: {len(w['code'])} lines {res} {'identical' if same else 'DIFFERENT'}")
        if not same:
            rc = 1
            if a.v:
                if o["meta"] != w["meta"] or o["desc"] != w["desc"]:
                    print("  old:", o["meta"], "\n  new:", w["meta"])
                    for d in list(difflib.unified_diff(o["desc"], w["desc"], lineterm="", n=0))[:20]:
                        print("  " + d)
                for d in list(difflib.unified_diff(o["code"], w["code"], lineterm="", n=1))[:60]:
                    print("  " + d)
    return rc


if __name__ == "__main__":
    sys.exit(main())
