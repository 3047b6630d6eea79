#!/usr/bin/env python3
"""What a decode kernel does between its entry and its first weight load, read off the compiler's output: compiles
llama.swift_amd/csrc/decode.hip for gfx950 to assembly (device side only, the library's flags; no GPU needed) and prints for every
instance of k_gemv, k_qkv_attn and k_dec_attn_x
  kernarg      size of the kernel-argument block in bytes (.amdhsa_kernarg_size)
  lines        64-byte lines of it that are loaded from along the path below
  instr        instructions on the shortest path through the kernel's control flow from its entry to the first weight load (a
               non-temporal 16-byte global load); `-` where the kernel has none
  waits        s_waitcnt on lgkmcnt along that path with scalar loads outstanding: the scalar round trips of the entry
  ka<nt        scalar loads from the kernarg segment along that path
  ka>bar       scalar loads from the kernarg segment that stand behind the first s_barrier in the text
A report, not a gate.
usage: kernel_entry_report.py [--asm decode.s] [--probe N] > profiles/entry_report_<tree>.txt"""
import argparse
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "llama.swift_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-x", "hip"]

ap = argparse.ArgumentParser()
ap.add_argument("--asm", help="read this assembly file instead of compiling")
ap.add_argument("--probe", type=int, default=0, help="compile with -DLH_PHASE_PROBE=N")
args = ap.parse_args()
if args.asm:
    text = open(args.asm).read()
else:
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "decode.s")
        cmd = [HIPCC] + FLAGS + ([f"-DLH_PHASE_PROBE={args.probe}"] if args.probe else []) + [os.path.join(CSRC, "decode.hip"), "-o", out]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()

lines = text.splitlines()
# kernel descriptors: name -> {directive: value}
desc, cur = {}, None
for ln in lines:
    s = ln.strip()
    if s.startswith(".amdhsa_kernel "):
        cur = s.split()[1]
        desc[cur] = {}
    elif s == ".end_amdhsa_kernel":
        cur = None
    elif cur and s.startswith(".amdhsa_"):
        p = s.split()
        if len(p) == 2:
            desc[cur][p[0]] = p[1]
names = sorted(desc)
dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
pretty = dict(zip(names, dem))
label_at = {}
for i, ln in enumerate(lines):
    m = re.match(r"^(\w+):", ln)
    if m and m.group(1) in desc:
        label_at.setdefault(m.group(1), i)


def kernarg_pair(d):
    """first SGPR of the kernarg segment pointer: user SGPRs are handed out in a fixed order"""
    at = 0
    for key, n in ((".amdhsa_user_sgpr_private_segment_buffer", 4), (".amdhsa_user_sgpr_dispatch_ptr", 2), (".amdhsa_user_sgpr_queue_ptr", 2)):
        if d.get(key, "0") == "1":
            at += n
    return at


def body(name):
    """the kernel's text as a list of instructions and of ("label", name) entries"""
    i = label_at[name]
    out = []
    for ln in lines[i + 1:]:
        s = ln.strip()
        if s.startswith(".Lfunc_end") or s.startswith(".section"):
            break
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            out.append(("label", m.group(1)))
        if not s or s[0] in ".;" or s.endswith(":"):
            continue
        out.append(s.split(";")[0].strip())
    return out


SREG = re.compile(r"s\[(\d+):(\d+)\]|s(\d+)")


def sregs(tok):
    m = SREG.fullmatch(tok.strip())
    if not m:
        return set()
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m.group(1) else {int(m.group(3))}


rows = []
for n in names:
    p = pretty[n]
    if not re.search(r"lh::(k_gemv<|k_qkv_attn<|k_dec_attn_x\()", p):
        continue
    short = re.sub(r"^void ", "", p)
    short = short[:short.index("(")]
    ka0 = kernarg_pair(desc[n])
    kbase = [{ka0, ka0 + 1}]                 # SGPR pairs that hold the kernarg pointer
    ksize = int(desc[n].get(".amdhsa_kernarg_size", "0"))
    items = body(n)
    labels = {it[1]: k for k, it in enumerate(items) if isinstance(it, tuple)}
    # text order: which scalar loads read the kernarg segment, and how many of them come after the first barrier
    is_ka, ka_after_bar, seen_bar = {}, 0, False
    for k, ins in enumerate(items):
        if isinstance(ins, tuple):
            continue
        op, _, rest = ins.partition(" ")
        ops = [o.strip() for o in rest.split(",")]
        is_ka[k] = op.startswith("s_load_dword") and len(ops) >= 3 and sregs(ops[1]) in kbase
        if op == "s_mov_b64" and len(ops) == 2 and sregs(ops[1]) in kbase:
            kbase.append(sregs(ops[0]))
        elif ops and op.startswith("s_") and not op.startswith(("s_cmp", "s_waitcnt", "s_cbranch", "s_branch", "s_barrier")):
            kbase = [b for b in kbase if not (b & sregs(ops[0]))]          # a pair that is written over no longer points at the arguments
        if op == "s_barrier":
            seen_bar = True
        if is_ka[k] and seen_bar:
            ka_after_bar += 1
    # the shortest path through the control-flow graph from the entry to a weight load (16 bytes per lane, non-temporal)
    def weight_load(ins):
        return not isinstance(ins, tuple) and ins.startswith("global_load_dwordx4") and re.search(r"\bnt\b", ins)
    prev, queue, goal = {0: None}, [0], None
    while queue and goal is None:
        nxt = []
        for k in queue:
            ins = items[k]
            if weight_load(ins):
                goal = k
                break
            succ = []
            op = "" if isinstance(ins, tuple) else ins.split(" ")[0]
            if op in ("s_branch",) or op.startswith("s_cbranch"):
                t = ins.split()[-1]
                if t in labels:
                    succ.append(labels[t])
            if op not in ("s_branch", "s_endpgm", "s_setpc_b64") and k + 1 < len(items):
                succ.append(k + 1)
            for t in succ:
                if t not in prev:
                    prev[t] = k
                    nxt.append(t)
        queue = nxt
    path = []
    k = goal
    while k is not None:
        path.append(k)
        k = prev[k]
    path.reverse()
    instr = waits = ka_before = pending = 0
    touched = set()
    for k in path[:-1]:
        ins = items[k]
        if isinstance(ins, tuple):
            continue
        instr += 1
        op, _, rest = ins.partition(" ")
        ops = [o.strip() for o in rest.split(",")]
        if op.startswith("s_load") or op.startswith("s_buffer_load"):
            pending += 1
        if is_ka[k]:
            ka_before += 1
            off = int(ops[2], 0) if re.fullmatch(r"0x[0-9a-f]+|\d+", ops[2]) else 0
            width = {"": 1, "x2": 2, "x3": 3, "x4": 4, "x8": 8, "x16": 16}.get(op[len("s_load_dword"):], 1)
            if off < ksize:
                touched.update(range(off // 64, (off + 4 * width - 1) // 64 + 1))
        if op == "s_waitcnt" and "lgkmcnt" in rest:
            waits += 1 if pending else 0
            pending = 0
    rows.append((short, ksize, len(touched), instr if goal is not None else None, waits, ka_before, ka_after_bar))

print(f"# decode.hip{' -DLH_PHASE_PROBE=%d' % args.probe if args.probe else ''} for gfx950: {len(rows)} decode kernel instances")
print("%-44s %7s %5s %6s %5s %5s %6s" % ("kernel", "kernarg", "lines", "instr", "waits", "ka<nt", "ka>bar"))
for r in sorted(rows):
    print("%-44s %7d %5d %6s %5d %5d %6d" % (r[0], r[1], r[2], "-" if r[3] is None else r[3], r[4], r[5], r[6]))
