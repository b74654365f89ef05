#!/usr/bin/env python3
"""Per-kernel comparison of the device code of two commits, for refactors that must not move it.

    scripts/device_code_compare.py --parent REV --out profiles/NAME.json [--what TEXT] [FILE.hip ...]

Each csrc/*.hip file (default: every one that includes kernel_args.hpp) is compiled to gfx950
assembly, device side only, with the Makefile's flags: once from REV (its csrc/ and include/ are
extracted with `git archive` into a temporary directory) and once from the working tree.  The text
is normalised, cut into kernels, and each kernel instantiation is reduced to an instruction count,
a digest and its resources.  A kernel's own symbol is written <self> in its text, so an instantiation
whose mangled name alone changed (a template parameter pack added behind the others, empty for it)
compares equal under its demangled name; --defaulted-arg VALUE does the same for a template argument added
behind the others with a default, --dropped-args N for the last N template arguments taken away (the
parent's instantiations that had 0 there), and --renamed OLD=NEW for a kernel that moved to another
template (prefixes of the demangled name).  An instantiation the parent does not have is listed as
added ("identical": null) and is no difference.  The order of the kernels in each file's assembly -- the
code object's order -- is compared too ("order_identical", over the kernels both commits have).
Needs hipcc and git, no GPU.  Exit status 1 when anything differs.
"""
import argparse
import hashlib
import io
import json
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "iib_project_ldpc_codes_amd/csrc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]
HOW = ("hipcc --offload-arch=gfx950 --cuda-device-only -S with the Makefile's flags (" + " ".join(FLAGS) + ") on each "
       "file at each commit; .file / .ident lines, comments, the per-file __hip_cuid symbol and the function index "
       "inside block labels (.LBB<i>_) normalised away, the kernel's own symbol written <self>; per kernel the function body up to .Lfunc_end: instructions "
       "counted, SHA-256 of the normalised text (first 16 hex digits), resources from its .amdhsa_kernel block "
       "(next_free_vgpr, next_free_sgpr, accum_offset, static LDS, scratch).  Made by scripts/device_code_compare.py.")
RESOURCES = {"vgpr": "next_free_vgpr", "sgpr": "next_free_sgpr", "accum_offset": "accum_offset",
             "static_lds": "group_segment_fixed_size", "scratch": "private_segment_fixed_size"}


def assembly(tree, name):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S"] + FLAGS + [
        "-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, CSRC), os.path.join(tree, CSRC, name), "-o", "-"]
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout


def normalise(text):
    out = []
    for line in text.splitlines():
        line = line.split(";", 1)[0].rstrip()
        if not line.strip() or re.match(r"\s*\.(file|ident)\b", line):
            continue
        line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line)
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def demangle(symbols):
    if not symbols:
        return {}
    names = subprocess.run(["c++filt"] + symbols, check=True, stdout=subprocess.PIPE,
                           universal_newlines=True).stdout.splitlines()
    return dict(zip(symbols, names))


def kernels(text):
    """{demangled kernel: {instructions, digest, resources...}} of one file's assembly"""
    lines = normalise(text)
    res, sym = {}, None
    for line in lines:  # the .amdhsa_kernel blocks
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            sym = m.group(1)
            res[sym] = {}
        elif re.match(r"\s*\.end_amdhsa_kernel", line):
            sym = None
        elif sym:
            for key, field in RESOURCES.items():
                m = re.match(r"\s*\.amdhsa_" + field + r"\s+(\S+)", line)
                if m:
                    res[sym][key] = int(m.group(1), 0)
    found, body, sym = {}, None, None
    for line in lines:  # the function bodies of those symbols
        m = re.match(r"(\S+):$", line)
        if m and m.group(1) in res and body is None:
            sym, body = m.group(1), []
        elif body is not None and re.match(r"\.Lfunc_end\d+:", line):
            insns = [l for l in body if not re.match(r"\s*\.|\S+:$", l)]
            digest = hashlib.sha256("\n".join(body).replace(sym, "<self>").encode()).hexdigest()[:16]
            found[sym] = dict(instructions=len(insns), digest=digest, **{k: res[sym].get(k) for k in RESOURCES})
            body = None
        elif body is not None:
            body.append(line)
    names = demangle(sorted(found))
    return {names[s].replace("ldpc::(anonymous namespace)::", ""): v for s, v in found.items()}


def default_files():
    names = sorted(f for f in os.listdir(os.path.join(ROOT, CSRC)) if f.endswith(".hip"))
    return [f for f in names if '"kernel_args.hpp"' in open(os.path.join(ROOT, CSRC, f)).read()]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", required=True, help="the commit to compare the working tree with")
    ap.add_argument("--out", required=True)
    ap.add_argument("--what", default=None)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--defaulted-arg", default=None, metavar="VALUE",
                    help="a template argument added behind the others with this default: an instantiation that ends "
                         "', VALUE>' and that the parent lacks is compared with the parent's of the name without it")
    ap.add_argument("--dropped-args", type=int, default=0, metavar="N",
                    help="the last N template arguments were taken away: an instantiation that the parent lacks is "
                         "compared with the parent's of the same leading arguments and N times ', 0' behind them")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW",
                    help="a parent's kernel whose demangled name starts with OLD is compared under the name with NEW "
                         "in OLD's place (may be given more than once)")
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    files = a.files or default_files()
    with tempfile.TemporaryDirectory() as parent:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.parent, CSRC, "include"], check=True,
                             stdout=subprocess.PIPE).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(parent)
        jobs = [(tree, f) for f in files for tree in (parent, ROOT)]
        with ThreadPoolExecutor(a.jobs) as pool:
            texts = dict(zip(jobs, pool.map(lambda j: assembly(*j), jobs)))
    rows, orders = [], []
    for f in files:
        old, new = kernels(texts[(parent, f)]), kernels(texts[(ROOT, f)])
        if a.defaulted_arg is not None:  # the parent's instantiations under the names they have now
            tail = ", %s>(" % a.defaulted_arg
            was = {k.replace(tail, ">(", 1): k for k in new if k not in old and tail in k}
            old = {was.get(k, k): v for k, v in old.items()}
        for pair in a.renamed:
            was, now = pair.split("=", 1)
            old = {now + k[len(was):] if k.startswith(was) else k: v for k, v in old.items()}
        if a.dropped_args:
            tail = ", 0" * a.dropped_args + ">("
            was = {k.replace(">(", tail, 1): k for k in new if k not in old and k.replace(">(", tail, 1) in old}
            old = {was.get(k, k): v for k, v in old.items()}
        # dicts keep the assembly's order: the kernels both commits have must come in the same one
        orders.append([k for k in old if k in new] == [k for k in new if k in old])
        for k in sorted(set(old) | set(new)):
            rows.append({"file": f, "kernel": k, "parent": old.get(k), "new": new.get(k),
                         "identical": old[k] == new.get(k) if k in old else None})
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.parent], check=True, stdout=subprocess.PIPE,
                         universal_newlines=True).stdout.strip()
    doc = {"what": a.what or "Device code of %s at the parent commit and at this commit, per kernel instantiation."
           % ", ".join(files), "how": HOW, "parent": rev,
           "all_identical": all(r["identical"] for r in rows if r["parent"] is not None),
           "order_identical": all(orders),
           "instantiations": len(rows), "added": sum(r["parent"] is None for r in rows), "kernels": rows}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    differ = [r for r in rows if r["identical"] is False]
    for r in differ:
        print("DIFFERS", r["file"], r["kernel"])
    for f, same in zip(files, orders):
        if not same:
            print("ORDER DIFFERS", f)
    print("%d instantiations in %d files, %d added, %d differ" % (len(rows), len(files), doc["added"], len(differ)))
    return 1 if differ or not all(orders) else 0


if __name__ == "__main__":
    sys.exit(main())
