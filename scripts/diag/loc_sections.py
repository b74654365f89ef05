"""Static instruction counts of one bp_loc_chain_kernel / bp_loc_kernel instantiation by section of the compiler's assembly.

    python scripts/diag/loc_sections.py <kernels.s> [mangled-symbol-prefix]

<kernels.s>: `hipcc --offload-arch=gfx950 --cuda-device-only -S` of csrc/bp_loc_spa.hip with the Makefile's flags.
The default symbol is bp_loc_chain_kernel<5,512,TQ=500> (the bench code's).  The function is cut at its
s_barriers, in program order (chained kernel: before the first barrier the kernel's entry; then the staging; the
channel reads; initialisation with, behind it in program order, the rotated loop's variable phase; the check phase;
the posterior gathers; the scatter; the output tail with the substitution pass behind it), and the decode loop (the
depth-2 loop of the listing) is counted on its own.  Counts are static: a section that holds two alternative paths
(16-byte and narrow row I/O, the substitution pass) counts both.  Prints one JSON object.
"""
import collections
import json
import re
import sys

SYM = "_ZN4ldpc12_GLOBAL__N_119bp_loc_chain_kernelILi5ELi512ELi500EEEvNS_6BpArgsE"
KEYS = ("scratch_store", "scratch_load", "global_load", "global_store", "buffer_load", "buffer_store", "s_cbranch",
        "s_and_saveexec", "v_lshl_add_u64", "v_ashrrev_i32", "ds_write_b128", "ds_read_b128", "ds_write_b32",
        "ds_read_b32", "v_log", "v_exp", "v_rcp", "v_pk_", "v_readlane", "v_writelane", "s_nop")


def ops_of(lines):
    ins = [l.split(";")[0].strip() for l in lines if l.startswith("\t")]
    return [l.split()[0] for l in ins if l and not l.startswith(".")]


def count(ops):
    c = collections.Counter(ops)
    row = {"instructions": len(ops), "valu": sum(o.startswith("v_") and not o.startswith("v_readfirstlane") for o in ops),
           "branches": sum(o.startswith("s_cbranch") for o in ops)}
    row.update({k: sum(v for o, v in c.items() if o.startswith(k)) for k in KEYS if any(o.startswith(k) for o in c)})
    return row


def main():
    text = open(sys.argv[1]).read().split("\n")
    sym = sys.argv[2] if len(sys.argv) > 2 else SYM
    a = next(k for k, l in enumerate(text) if l.startswith(sym) and l.split(";")[0].rstrip().endswith(":"))
    b = next(k for k in range(a, len(text)) if text[k].startswith(".Lfunc_end"))
    body = text[a:b]
    ops = ops_of(body)
    bars = [k for k, o in enumerate(ops) if o == "s_barrier"]
    cuts = [0] + bars + [len(ops)]
    out = {"symbol": text[a].split(":")[0], "all": count(ops),
           "sections_between_barriers": [count(ops[cuts[i]:cuts[i + 1]]) for i in range(len(cuts) - 1)]}
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = (i, "Depth=2" in l or "Depth=2" in body[min(i + 1, len(body) - 1)])
    inner = sorted(i for i, d in labels.values() if d)
    back = [i for i, l in enumerate(body) for m in [re.match(r"\s+s_cbranch\S*\s+(\.LBB\d+_\d+)", l)]
            if m and labels.get(m.group(1), (0, False))[1] and labels[m.group(1)][0] <= i]
    loop = ops_of(body[inner[0]:max(back) + 1])
    out["decode_loop"] = count(loop)
    out["decode_loop_histogram"] = dict(sorted(collections.Counter(loop).items()))
    k = next(k for k, l in enumerate(text) if l.strip().startswith(".amdhsa_kernel " + out["symbol"]))
    for l in text[k:k + 90]:
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size)\s+(\S+)", l)
        if m:
            out[m.group(1)] = int(m.group(2), 0)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
