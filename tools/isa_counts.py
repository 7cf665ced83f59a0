#!/usr/bin/env python3
"""Static instruction counts of the field-product kernels, from the gfx950 ISA.

Compiles reef_amd/csrc/kernels_pallas.hip for the device only, with the Makefile's flags, and
prints for k_bench_fmul<0> (and for its loop body, which is 2 Montgomery products) and for the
bucket-accumulation kernels k_accum0<0,...> the VALU instruction count, the counts of the
instructions the product is made of, and the VGPR count and occupancy the compiler reports.
Works without a GPU.

    python tools/isa_counts.py [SOURCE_ROOT] [--json OUT]

SOURCE_ROOT defaults to this repository; point it at another checkout to compare two trees.
"""
import argparse
import collections
import json
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-pass-failed", "-fno-slp-vectorize",
         "-mllvm", "-amdgpu-load-store-vectorizer=0"]
TRACKED = ["v_mad_u64_u32", "v_lshrrev_b64", "v_lshl_add_u64", "v_and_b32", "v_sub_u32", "v_not_b32", "v_bfi_b32",
           "v_add_u32", "v_add_co_u32", "v_addc_co_u32", "v_cndmask_b32", "v_mov_b32", "s_nop"]


def compile_asm(src_root):
    csrc = os.path.join(src_root, "reef_amd", "csrc")
    out = os.path.join(tempfile.mkdtemp(prefix="isa_counts_"), "pallas.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + ["--offload-device-only", "-S", "-I" + csrc,
                           os.path.join(csrc, "kernels_pallas.hip"), "-o", out])
    return open(out).read()


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, p.stdout.splitlines()))


def functions(asm):
    """{mangled name: lines of its body} for every kernel in the assembly."""
    funcs, cur, body = {}, None, []
    for line in asm.splitlines():
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if re.match(r"^\s*\.Lfunc_end", line) or re.match(r"^\.Lfunc_end", line):
            funcs[cur] = body
            cur = None
            continue
        body.append(line)
    return funcs


def stats(asm, name):
    body = functions(asm)[name]
    ops = collections.Counter()
    for line in body:
        s = line.strip()
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        ops[s.split()[0].split("_e32")[0].split("_e64")[0]] += 1
    valu = sum(v for k, v in ops.items() if k.startswith("v_"))
    meta = {}
    tail = asm[asm.index(".size\t%s, .Lfunc_end" % name):]   # the compiler's register and occupancy notes follow the body
    for key in ("NumVgprs", "Occupancy", "ScratchSize"):
        m = re.search(r";\s*%s:\s*(\d+)" % key, tail)
        if m:
            meta[key] = int(m.group(1))
    return {"valu": valu, "ops": {k: ops.get(k, 0) for k in TRACKED}, **meta}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src_root", nargs="?", default=ROOT)
    ap.add_argument("--json")
    a = ap.parse_args()
    asm = compile_asm(a.src_root)
    names = [n for n in functions(asm) if "k_bench_fmul" in n or "k_accum0" in n]
    pretty = demangle(names)
    res = {}
    for n in sorted(names, key=lambda n: pretty[n]):
        if "k_accum0" in pretty[n] and not pretty[n].split("(")[0].startswith("void reef::k_accum0<0"):
            continue
        res[pretty[n].split("(")[0].replace("void reef::", "")] = stats(asm, n)
    for k, v in res.items():
        print(f"{k}: VALU {v['valu']}  VGPRs {v.get('NumVgprs')}  occupancy {v.get('Occupancy')}")
        print("    " + "  ".join(f"{op} {c}" for op, c in v["ops"].items() if c))
    loop = fmul_loop(asm, [n for n in names if "k_bench_fmul" in n][0])
    print("k_bench_fmul<0> loop body (2 products): " + "  ".join(f"{op} {c}" for op, c in loop.items() if c)
          + f"  VALU {sum(c for op, c in loop.items() if op.startswith('v_'))}")
    res["k_bench_fmul<0>:loop"] = dict(loop)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


def fmul_loop(asm, name):
    """Instruction counts of the k_bench_fmul loop: the basic block that ends in the backward branch."""
    body = functions(asm)[name]
    blocks, cur, label = {}, [], None
    for line in body:
        s = line.strip()
        m = re.match(r"^(\.LBB\S+):", s)
        if m:
            if label:
                blocks[label] = cur
            label, cur = m.group(1), []
            continue
        if s and not s.startswith((";", ".")):
            cur.append(s)
    if label:
        blocks[label] = cur
    for lab, ins in blocks.items():
        if any(i.startswith("s_cbranch") and lab in i for i in ins):
            ops = collections.Counter(i.split()[0].split("_e32")[0].split("_e64")[0] for i in ins)
            return collections.OrderedDict(sorted(ops.items(), key=lambda kv: -kv[1]))
    raise SystemExit("k_bench_fmul: loop block not found")


if __name__ == "__main__":
    main()
