#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the device assembly of two builds of csrc/*.hip.

    python tools/isa_diff.py REV [-o report.txt] [-j N]

Builds the csrc/ of git revision REV and the working tree's into two temporary directories with the Makefile's own flags
(`make print-flags`) plus --save-temps, and compares what the compiler emitted for every kernel.  Runs on the build
machine; it needs hipcc and no GPU.

A kernel is keyed by its mangled name, not by its file, so a kernel that moved to another .hip file is still compared
with its counterpart.  Its text is everything from its label to its .Lfunc_end, the .amdhsa_ block included, with
comments and .loc / .file / .ident / .cfi lines dropped and the function's ordinal taken out of local labels
(.LBB<n>_<m>, .Lfunc_end<n>, .Ltmp<n>, .LJTI<n>_<m>): those depend only on where in its file a kernel stands.  What
is left is compared as plain text.  The resource figures come from the code object's metadata, the code size from the
compiler's own "codeLenInByte" note.  Exit status 1 when some kernel differs, is missing or is new.
"""
import argparse
import concurrent.futures
import difflib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "mt_renderer_amd/csrc"
FIGS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")

_LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp|LJTI|LCPI)\d+")
_DROP = re.compile(r"^\s*\.(loc|file|ident|cfi_\w+)\b")


def normalise(lines):
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip() or _DROP.match(ln):
            continue
        out.append(_LABEL.sub(lambda m: "." + m.group(1), ln))
    return out


def parse_asm(path, obj):
    """{mangled kernel name: {"obj", "text", figures..., "code_bytes"}} of one device .s file"""
    with open(path) as f:
        lines = f.read().split("\n")
    kernels = {}
    names = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    starts = {ln.split(":", 1)[0]: i for i, ln in enumerate(lines) if ln[:1] not in ("\t", " ", ".", ";", "") and ":" in ln}
    for name in names:
        i0 = starts[name]
        i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
        size = next(int(m.group(1)) for ln in lines[i1:] for m in [re.match(r"; codeLenInByte = (\d+)", ln)] if m)
        kernels[name] = {"obj": obj, "text": normalise(lines[i0 : i1 + 1]), "code_bytes": size}
    # metadata: a YAML list of kernels, every figure before or after its .name inside one "  - " item
    meta = lines[lines.index("amdhsa.kernels:") :] if "amdhsa.kernels:" in lines else []
    item = {}
    for ln in meta + ["  - "]:
        if ln.startswith("  - ") or ln.startswith("amdhsa.target"):
            if "name" in item:
                kernels[item["name"]].update({k: int(item[k]) for k in FIGS})
            item = {}
            ln = "    " + ln[4:]
        m = re.match(r"    \.(\w+):\s+(\S+)$", ln)
        if m:
            item[m.group(1)] = m.group(2)
    return kernels


def build(srcdir, outdir, flags, jobs):
    """compiles every .hip of srcdir in outdir and returns the kernels of all of them"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    srcs = sorted(f for f in os.listdir(srcdir) if f.endswith(".hip"))

    def one(src):
        d = os.path.join(outdir, src[:-4])
        os.makedirs(d)
        cmd = [hipcc] + flags + ["--save-temps", "-c", os.path.join(srcdir, src), "-o", src[:-4] + ".o"]
        r = subprocess.run(cmd, cwd=d, capture_output=True, text=True)
        if r.returncode:
            sys.exit("build of %s failed:\n%s" % (os.path.join(srcdir, src), r.stderr))
        asm = [f for f in os.listdir(d) if "amdgcn" in f and f.endswith(".s")]
        return parse_asm(os.path.join(d, asm[0]), src[:-4] + ".o")

    kernels = {}
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        for k in ex.map(one, srcs):
            kernels.update(k)
    return kernels


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev", help="git revision to compare the working tree against")
    ap.add_argument("-o", "--output", help="also write the report to this file")
    ap.add_argument("-j", "--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()

    flags = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, CSRC), "print-flags"], capture_output=True, text=True,
                           check=True).stdout.split()
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", args.rev], capture_output=True, text=True, check=True).stdout.strip()
    with tempfile.TemporaryDirectory(prefix="isa_diff_") as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.rev, CSRC], capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.join(tmp, "rev_src"))
        old = build(os.path.join(tmp, "rev_src", CSRC), os.path.join(tmp, "rev"), flags, args.jobs)
        new = build(os.path.join(ROOT, CSRC), os.path.join(tmp, "tree"), flags, args.jobs)

    pretty = demangle(sorted(set(old) | set(new)))
    out = ["# device assembly of csrc/*.hip: working tree against %s, per kernel" % rev,
           "# flags: %s --save-temps" % " ".join(flags),
           "# figures: vgpr_count sgpr_count private_segment_fixed_size group_segment_fixed_size code_bytes (%s -> tree)" % rev, ""]
    bad = 0
    fig = lambda k: " ".join(str(k[f]) for f in FIGS + ("code_bytes",))
    for name in sorted(set(old) | set(new), key=lambda n: ((new.get(n) or old[n])["obj"], pretty[n])):
        o, n = old.get(name), new.get(name)
        if o is None or n is None:
            verdict, bad = ("new" if o is None else "missing"), bad + 1
        elif o["text"] == n["text"]:
            verdict = "identical"
        else:
            d = [ln[0] for ln in difflib.unified_diff(o["text"], n["text"], n=0, lineterm="") if ln[:2] not in ("--", "++", "@@")]
            verdict, bad = "differs (%d -> %d lines: -%d +%d)" % (len(o["text"]), len(n["text"]), d.count("-"), d.count("+")), bad + 1
        where = (n or o)["obj"] if not (o and n) or o["obj"] == n["obj"] else "%s -> %s" % (o["obj"], n["obj"])
        out.append("%-10s %s  [%s]" % (verdict.split(" ")[0], pretty[name], where))
        if verdict.startswith("differs"):
            out.append("           %s" % verdict)
        out.append("           %s" % name)
        out.append("           %s  ->  %s" % (fig(o) if o else "-", fig(n) if n else "-"))
    out.append("")
    out.append("%d kernels, %d not identical" % (len(set(old) | set(new)), bad))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.output:
        with open(args.output, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
