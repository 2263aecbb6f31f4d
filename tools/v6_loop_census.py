#!/usr/bin/env python3
"""Instruction census of the k_gru_steps_v6 task loop, from a gfx950 cross-compile.  Needs no GPU.

    python tools/v6_loop_census.py                  # compile csrc/cvae_lib.hip to assembly with the build's flags, print every instance
    python tools/v6_loop_census.py --asm FILE.s     # read an assembly file made earlier (e.g. of another commit)
    python tools/v6_loop_census.py --only 16,8,3,0,0

A step of the recurrence is bound by the wave's own instruction stream (one wave per SIMD: DESIGN.md 4.1), so what the
compiler puts between the MFMAs is what a step costs.  The task loop of an instance is fully unrolled inside; its body is
cut into three stretches by counting MFMAs (6 per 16-k step with three limbs, 3 with two):

    front-end   loop header .. the last of the KFW * n front-end MFMAs
    recurrent   from there .. the last of the KPW * n recurrent MFMAs (the flag poll and the operand requests are in here;
                the poll's own inner loops are left out of the counts: they run an unknown number of times)
    reduction   from there .. the first s_barrier (accumulator reads, the limb sum, the LDS writes)

and for each stretch the tool counts MFMAs, v_accvgpr_read_b32 / v_accvgpr_write_b32, other VALU, SALU, s_waitcnt by
counter, and clock reads (s_memtime / s_memrealtime).  Per kernel: next_free_vgpr, accum_offset, scratch bytes per lane.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cyclevae-vc_amd", "csrc")
NAME = re.compile(r"^_Z14k_gru_steps_v6ILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E(?:Lb([01])E)?Ev11Step6Params$")
STRETCHES = ("front-end", "recurrent", "reduction")


def compile_asm(out):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    # the flags of __graft_entry__.build(), with the device assembly as the product
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           "--cuda-device-only", "-S", os.path.join(CSRC, "cvae_lib.hip"), "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def kernels(path):
    """{mangled name: (lines of the body, {directive: value})} for every k_gru_steps_v6 instance of the file"""
    out, meta, name, desc = {}, {}, None, None
    with open(path) as f:
        for raw in f:
            line = raw.rstrip("\n")
            # the kernel descriptor (.amdhsa_kernel ... .end_amdhsa_kernel) sits behind the code, in front of the .size line
            m = re.match(r"^\s+\.amdhsa_kernel\s+(\S+)", line)
            if m:
                desc = m.group(1) if NAME.match(m.group(1)) else None
                name = None
                continue
            if ".end_amdhsa_kernel" in line:
                desc = None
                continue
            if desc:
                m = re.match(r"^\s+\.amdhsa_(next_free_vgpr|accum_offset|private_segment_fixed_size)\s+(\d+)", line)
                if m:
                    meta.setdefault(desc, {})[m.group(1)] = int(m.group(2))
                continue
            m = re.match(r"^(_Z14k_gru_steps_v6\w+):", line)
            if m and NAME.match(m.group(1)):
                name = m.group(1)
                out[name] = []
            elif name and (line.startswith(".Lfunc_end") or re.match(r"^\s+\.(size|section)\s", line)):
                name = None
            elif name:
                out[name].append(line)
    return {k: (v, meta.get(k, {})) for k, v in out.items()}


def _insn(line):
    s = line.split(";")[0].strip()
    if not s or s.endswith(":") or s.startswith("."):
        return None
    return s


def _blocks(body):
    """[(label or None, depth, [instructions])]: depth from the compiler's loop comments (0 outside any loop)"""
    blocks, cur = [], [None, 0, []]
    for line in body:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", line)
        if m:
            blocks.append(tuple(cur))
            c = m.group(2) or ""
            d = re.search(r"Depth=(\d+)", c)
            cur = [m.group(1), int(d.group(1)) if d else 0, []]
            continue
        i = _insn(line)
        if i:
            cur[2].append(i)
    blocks.append(tuple(cur))
    return blocks


def _empty():
    return {"mfma": 0, "accvgpr_read": 0, "accvgpr_write": 0, "valu_other": 0, "salu": 0, "clock": 0,
            "ds_read": 0, "vmem_load": 0, "waitcnt": {}}


def _count(c, insn):
    op = insn.split()[0]
    if op.startswith("v_mfma"):
        c["mfma"] += 1
    elif op == "v_accvgpr_read_b32":
        c["accvgpr_read"] += 1
    elif op == "v_accvgpr_write_b32":
        c["accvgpr_write"] += 1
    elif op.startswith("v_"):
        c["valu_other"] += 1
    elif op == "s_waitcnt":
        for kind, n in re.findall(r"(vmcnt|lgkmcnt|expcnt)\((\d+)\)", insn):
            key = "%s(%s)" % (kind, n)
            c["waitcnt"][key] = c["waitcnt"].get(key, 0) + 1
    elif op in ("s_memtime", "s_memrealtime") or (op == "s_getreg_b32" and "SHADER_CYCLES" in insn):
        c["clock"] += 1
    elif op.startswith("s_"):
        c["salu"] += 1
    elif op.startswith("ds_read") or op.startswith("ds_load"):
        c["ds_read"] += 1
    elif op.startswith(("buffer_load", "global_load", "flat_load")):
        c["vmem_load"] += 1


def census(name, body, meta):
    kpw, kfw, limbs, w2s, prof = NAME.match(name).groups()
    kpw, kfw, limbs = int(kpw), int(kfw), int(limbs)
    per = 6 if limbs == 3 else 3
    n_fe, n_rec = kfw * per, kpw * per
    res = {"name": name, "KPW": kpw, "KFW": kfw, "LIMBS": limbs, "W2S": w2s == "1", "PROF": prof == "1",
           "next_free_vgpr": meta.get("next_free_vgpr"), "accum_offset": meta.get("accum_offset"),
           "scratch": meta.get("private_segment_fixed_size"), "stretch": {k: _empty() for k in STRETCHES}}
    # the task loop: the depth-1 loop that holds the MFMAs.  Its blocks in layout order; inner loops (depth >= 2) are the polls
    blocks = _blocks(body)
    first = next((n for n, b in enumerate(blocks) if b[1] >= 1 and any(i.startswith("v_mfma") for i in b[2])), None)
    if first is None:
        res["error"] = "no MFMA inside a loop"
        return res
    # walk back to the loop header: the first depth >= 1 block of the run of loop blocks that contains `first`
    start = first
    while start > 0 and blocks[start - 1][1] >= 1:
        start -= 1
    seen, stage = 0, 0
    for b in blocks[start:]:
        if b[1] < 1:
            break
        for insn in b[2]:
            if stage > 2:
                break
            if b[1] >= 2:
                continue
            if stage == 2 and insn.startswith("s_barrier"):
                stage = 3
                break
            _count(res["stretch"][STRETCHES[stage]], insn)
            if insn.startswith("v_mfma"):
                seen += 1
                if stage == 0 and seen == n_fe:
                    stage = 1
                if stage == 1 and seen == n_fe + n_rec:
                    stage = 2
            if stage == 0 and n_fe == 0:
                stage = 1
    res["task_loop_mfma"] = seen
    if seen != n_fe + n_rec:
        res["error"] = "expected %d MFMAs in the task loop, counted %d" % (n_fe + n_rec, seen)
    # every clock read of the loop, wherever it sits (also behind the reduction)
    res["task_loop_clock"] = sum(1 for b in blocks[start:] if b[1] >= 1 for i in b[2]
                                 if i.split()[0] in ("s_memtime", "s_memrealtime"))
    return res


def run(asm=None, only=None):
    tmp = None
    if asm is None:
        tmp = tempfile.NamedTemporaryFile(suffix=".s", delete=False)
        tmp.close()
        asm = tmp.name
        compile_asm(asm)
    try:
        ks = kernels(asm)
    finally:
        if tmp:
            os.unlink(tmp.name)
    out = []
    for name in sorted(ks):
        g = NAME.match(name).groups()
        key = ",".join(x if x is not None else "0" for x in g)
        if only and key != only:
            continue
        r = census(name, *ks[name])
        r["key"] = key
        out.append(r)
    return out


def fmt(r):
    lines = ["k_gru_steps_v6<%s>  next_free_vgpr %s  accum_offset %s  scratch %s%s" %
             (r["key"], r["next_free_vgpr"], r["accum_offset"], r["scratch"], "  !! " + r["error"] if "error" in r else "")]
    lines.append("  %-10s %5s %8s %9s %6s %5s %6s %8s %6s  %s" %
                 ("stretch", "mfma", "acc_read", "acc_write", "valu", "salu", "clock", "ds_read", "vmem", "s_waitcnt"))
    for k in STRETCHES:
        c = r["stretch"][k]
        w = " ".join("%s x%d" % kv for kv in sorted(c["waitcnt"].items()))
        lines.append("  %-10s %5d %8d %9d %6d %5d %6d %8d %6d  %s" %
                     (k, c["mfma"], c["accvgpr_read"], c["accvgpr_write"], c["valu_other"], c["salu"], c["clock"],
                      c["ds_read"], c["vmem_load"], w))
    lines.append("  clock reads anywhere in the task loop: %d" % r["task_loop_clock"])
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="assembly file to read instead of compiling")
    ap.add_argument("--only", help="one instance: KPW,KFW,LIMBS,W2S,PROF (0/1)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    rs = run(a.asm, a.only)
    if a.json:
        print(json.dumps(rs, indent=1))
    else:
        print("\n".join(fmt(r) for r in rs))
    return 0


if __name__ == "__main__":
    sys.exit(main())
