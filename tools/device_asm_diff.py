"""Compare the gfx950 device code of two versions of one HIP source, kernel by kernel.

    python tools/device_asm_diff.py OLD.hip NEW.hip [--include-old DIR] [--rename OLD_NAME=NEW_NAME ...]

Both files are compiled with the library's flags (__graft_entry__.FLAGS) plus --cuda-device-only -S; OLD.hip with -I DIR in front
(the headers of the commit it comes from; default: its own directory).  Comment lines, .file / .loc / .ident lines and the
__hip_cuid_* lines are dropped, names are demangled, --rename maps the old names of renamed types, and local labels lose their
function number.  Per kernel the instruction stream (label to .Lfunc_end) and the .amdhsa_kernel block (registers, LDS, scratch)
are compared; every difference is printed as a unified diff.  Exit status 0 and "N kernels, all identical" = no difference."""
import argparse
import difflib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import FLAGS, HIPCC  # noqa: E402

CXXFILT = "c++filt"


def device_asm(src, include=None):
    flags = [f for f in FLAGS if f != "-fPIC"]
    cmd = [HIPCC, "--cuda-device-only", "-S", src, "-o", "-"] + (["-I" + include] if include else []) + flags
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    text = subprocess.run([CXXFILT], input=text, check=True, capture_output=True, text=True).stdout
    keep = []
    for line in text.splitlines():
        s = line.strip()
        if not s or s.startswith(";") or s.startswith((".file", ".loc", ".ident", ".section")) or "__hip_cuid_" in s:
            continue
        line = re.sub(r"\s*;.*$", "", line.rstrip()).replace("> >", ">>")
        keep.append(re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+", r".\1", line))
    return keep


def kernels(lines, renames):
    """{kernel name: its code lines + its .amdhsa_kernel block}"""
    for old, new in renames:
        lines = [ln.replace(old, new) for ln in lines]
    out, name = {}, None
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (.+)$", ln)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            out.setdefault(m.group(1), []).extend(lines[i:end + 1])
        m = re.match(r"(\S.*):$", ln)
        if m and not ln.startswith("."):
            name = m.group(1)
            out.setdefault(name, [])
        if name is not None:
            out[name].append(ln)
            if ln.strip().startswith(".Lfunc_end"):
                name = None
    return {k: v for k, v in out.items() if any(x.strip().startswith(".amdhsa_kernel") for x in v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--include-old", default=None)
    ap.add_argument("--rename", action="append", default=[])
    a = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in a.rename]
    old = kernels(device_asm(a.old, a.include_old or os.path.dirname(os.path.abspath(a.old))), renames)
    new = kernels(device_asm(a.new), [])
    bad = sorted(set(old) ^ set(new))
    for k in bad:
        print("only in %s: %s" % ("old" if k in old else "new", k))
    for k in sorted(set(old) & set(new)):
        if old[k] != new[k]:
            bad.append(k)
            sys.stdout.write("\n".join(difflib.unified_diff(old[k], new[k], "old " + k, "new " + k, lineterm="", n=2)) + "\n")
    print("%d kernels, %s" % (len(new), "all identical" if not bad else "%d differ" % len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
