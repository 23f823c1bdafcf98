#!/usr/bin/env python3
"""Device code of the conv stack's units against a reference source, kernel by kernel, without a GPU.

    python scripts/conv_units_isa.py --ref-rev <commit> [--ref-file crnn-ocr-lite_amd/csrc/conv.hip] [-o profiles/conv_units_refactor.txt]
    python scripts/conv_units_isa.py --ref-rev <commit> --units dwconv_stream.hip,dwconv_bwd_stream.hip [-o ...]

Compiles the reference file as it stood at <commit> and the five units of today's tree -- with --units: each named unit of csrc/ as it stood at <commit> and
as it is today -- (hipcc --offload-arch=gfx950 -O3 -std=c++17 -S
--cuda-device-only -Rpass-analysis=kernel-resource-usage), cuts each assembly into one body per function symbol (the instructions and the kernel
descriptor), normalises what depends only on the file (local label numbers: .LBB<function>_<n>, .Lfunc_end<n>), and reports: the symbols missing, new or
defined twice, the bodies that differ in anything but comments (with a unified diff), and the resource remarks (VGPRs, AGPRs, SGPRs, scratch, LDS) that differ."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crnn-ocr-lite_amd", "csrc")
UNITS = ["dwconv_tile.hip", "reduce.hip", "batchnorm.hip", "elementwise.hip", "block1.hip"]
RES_KEYS = ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "SGPRs Spill", "VGPRs Spill")


def compile_unit(src, incs):
    """-> (assembly text, {kernel: {remark: value}})"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
        for i in incs:
            cmd += ["-I", i]
        r = subprocess.run(cmd + [src, "-o", out], capture_output=True, text=True)
        if r.returncode:
            sys.exit("hipcc failed on %s:\n%s" % (src, r.stderr[-3000:]))
        text = open(out).read()
    res, cur = {}, None
    for line in r.stderr.split("\n"):
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}(.+?): (\d+)\s*$", line)
        if m and cur is not None and m.group(1) in RES_KEYS:
            cur[m.group(1)] = int(m.group(2))
    return text, res


def bodies(text):
    """-> {symbol: [normalised lines]}: the function's instructions and, for a kernel, its descriptor block"""
    out = {}
    lines = text.split("\n")
    # (comments go: they repeat the label numbers -- "in Loop: Header=BB33_6" -- and are padded to the label's width)
    norm = lambda s: re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", re.sub(r"\.LBB\d+_", ".LBB_", s.split(";")[0])).rstrip()
    funcs = set(re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M))
    i = 0
    while i < len(lines):
        m = re.match(r"^(\w+):\s*(;.*)?$", lines[i])
        if m and m.group(1) in funcs:
            sym, j = m.group(1), i + 1
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            assert sym not in out, "symbol cut twice from one file: " + sym
            out[sym] = [norm(l) for l in lines[i:j]]
            i = j
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", lines[i]) if i < len(lines) else None
        if m:
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            out[m.group(1)] += ["<descriptor>"] + [norm(l) for l in lines[i:j + 1]]
            i = j
        i += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-rev", required=True)
    ap.add_argument("--ref-file", default="crnn-ocr-lite_amd/csrc/conv.hip")
    ap.add_argument("--units", default=None, help="comma-separated units of csrc/: compare each against the same path at --ref-rev")
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    units = a.units.split(",") if a.units else UNITS
    ref_files = ["crnn-ocr-lite_amd/csrc/" + u for u in units] if a.units else [a.ref_file]
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as td:   # the reference source with the headers of its own revision
        for f in subprocess.check_output(["git", "ls-tree", "--name-only", a.ref_rev, "crnn-ocr-lite_amd/csrc/", "include/"], cwd=ROOT, text=True).split():
            if f.endswith((".h", ".inc")) or f in ref_files:
                dst = os.path.join(td, f)
                os.makedirs(os.path.dirname(dst), exist_ok=True)
                open(dst, "wb").write(subprocess.check_output(["git", "show", "%s:%s" % (a.ref_rev, f)], cwd=ROOT))
        ref, ref_res = {}, {}
        for rf in ref_files:
            text, res = compile_unit(os.path.join(td, rf), [os.path.join(td, "include"), os.path.dirname(os.path.join(td, rf))])
            for sym, body in bodies(text).items():
                assert sym not in ref, "symbol defined by two reference files: " + sym
                ref[sym] = body
            ref_res.update(res)
    new, new_res, where, twice = {}, {}, {}, []
    for u in units:
        text, res = compile_unit(os.path.join(CSRC, u), [inc])
        for sym, body in bodies(text).items():
            if sym in new:
                twice.append((sym, where[sym], u))
            new[sym], where[sym] = body, u
        new_res.update(res)
    rep = []
    rep.append("reference: %s at %s; units: %s" % (", ".join(ref_files), a.ref_rev, ", ".join(units)))
    rep.append("function symbols: reference %d, units %d; missing %d, new %d, defined twice %d" %
               (len(ref), len(new), len(set(ref) - set(new)), len(set(new) - set(ref)), len(twice)))
    for s in sorted(set(ref) - set(new)):
        rep.append("  missing: " + s)
    for s in sorted(set(new) - set(ref)):
        rep.append("  new: %s (%s)" % (s, where[s]))
    for s, u1, u2 in twice:
        rep.append("  twice: %s (%s, %s)" % (s, u1, u2))
    common = sorted(set(ref) & set(new))
    same = [s for s in common if ref[s] == new[s]]
    rep.append("bodies compared %d, identical %d" % (len(common), len(same)))
    for s in common:
        if ref[s] != new[s]:
            rep.append("  differs: %s (%s)" % (s, where[s]))
            rep += ["    " + l for l in difflib.unified_diff(ref[s], new[s], "reference", where[s], lineterm="", n=1)][:80]
    kern = sorted(set(ref_res) & set(new_res))
    rsame = [s for s in kern if ref_res[s] == new_res[s]]
    rep.append("resource remarks (%s): kernels compared %d (reference %d, units %d), identical %d" %
               (", ".join(RES_KEYS), len(kern), len(ref_res), len(new_res), len(rsame)))
    for s in kern:
        if ref_res[s] != new_res[s]:
            rep.append("  differs: %s: %s -> %s" % (s, ref_res[s], new_res[s]))
    per = {}
    for s in common:
        per.setdefault(where[s], []).append(s)
    for u in units:
        rep.append("%-18s %3d functions, %5d instruction lines" % (u, len(per.get(u, [])), sum(len(new[s]) for s in per.get(u, []))))
    text = "\n".join(rep) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    ok = not (set(ref) ^ set(new)) and not twice and len(same) == len(common) and len(rsame) == len(kern) and len(kern) == len(ref_res) == len(new_res)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
