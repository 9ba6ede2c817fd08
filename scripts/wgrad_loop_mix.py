#!/usr/bin/env python3
"""Static instruction mix of the tile loop of a k_conv3d_wgrad_x16 instantiation, from the
assembly that `hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S conv3d_wgx.hip` writes:

    python scripts/wgrad_loop_mix.py conv3d_wgx.s 'ILi3ELi16ELi12ELi7ELb0ELi32ELb0E' [-v]

The tile loop is the outermost loop that holds the kernel's MFMAs;
the MFMA loops are the loops inside it that hold MFMAs (both from the compiler's loop
comments on the basic blocks).  The script counts, per basic block
of the tile loop outside the MFMA loops, the VALU, SALU, branch, exec-mask, global-load and
LDS instructions, and the MFMAs inside the MFMA loops.  Both arms of a uniform branch are
counted (the 7- and the 6-row-block preludes, for instance), so the sums are an upper bound
of what one tile executes.  Blocks that run once per column (the column's lane state and its
extra plane loads, behind uniform branches) are summed apart when their labels are given
with -c LABEL,LABEL...; -v prints the per-block table to pick them from.  It reports counts
only."""
import argparse
import re
import sys

ap = argparse.ArgumentParser()
ap.add_argument("asm")
ap.add_argument("kernel", help="substring of the mangled kernel name")
ap.add_argument("-v", action="store_true", help="per-block table")
ap.add_argument("-c", default="", help="comma-separated labels of per-column blocks")
a = ap.parse_args()

lines = open(a.asm).read().split("\n")
start = next(i for i, l in enumerate(lines)
             if l.startswith("_Z") and "wgrad_x16" in l and a.kernel in l
             and l.split(";")[0].strip().endswith(":"))
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
body = lines[start:end + 1]

# Basic blocks with the loop the compiler's comments put them in: "in Loop: Header=BBf_h
# Depth=d", "=>This Loop Header: Depth=1", "Parent Loop BBf_h" + "Inner Loop Header".
blk_re = re.compile(r"^(?:\.LBB\d+_(\d+):|; %bb\.(\d+):)")
ins = []      # (index, text, block)
first = {}    # block -> index of its first instruction
note = {}     # block -> loop comment text
cur, fresh = "entry", False
for l in body:
    st = l.strip()
    m = blk_re.match(st)
    if m:
        cur = ".LBB_" + (m.group(1) or m.group(2))
        first[cur] = len(ins)
        note[cur] = st
        fresh = True
        continue
    if st.startswith(";") and fresh:
        note[cur] += " " + st
        continue
    t = l.split(";")[0].strip()
    if not t or t.startswith(".") or t.endswith(":"):
        continue
    fresh = False
    ins.append((len(ins), t, cur))

top, inner_of, parent = {}, {}, {}
for b, n in note.items():
    num = b.split("_")[1]
    if "This Loop Header: Depth=1" in n:
        top[b] = num
    m = re.search(r"Parent Loop BB\d+_(\d+) Depth=1", n)
    if m and "Inner Loop Header: Depth=2" in n:
        top[b], inner_of[b], parent[num] = m.group(1), num, m.group(1)
    m = re.search(r"in Loop: Header=BB\d+_(\d+) Depth=1", n)
    if m:
        top[b] = m.group(1)
for b, n in note.items():
    m = re.search(r"in Loop: Header=BB\d+_(\d+) Depth=2", n)
    if m and m.group(1) in parent:
        top[b], inner_of[b] = parent[m.group(1)], m.group(1)

mf = [i for i, t, _ in ins if t.startswith("v_mfma")]
if not mf:
    sys.exit("no MFMA in this kernel")
heads = [top.get(ins[i][2]) for i in mf]
H = max(set(heads), key=heads.count)
if H is None:
    sys.exit("the MFMAs are in no loop")
inloop = {b for b in first if top.get(b) == H}
# blocks the comments leave out but a branch from inside the loop reaches backwards (the
# block in front of the header that the latch re-enters through)
hpos = first[".LBB_" + H]
order_all = sorted(first, key=first.get)
for i, t, b in ins:
    m = re.match(r"^s_c?branch\S*\s+\.LBB\d+_(\d+)", t)
    if m and b in inloop:
        tgt = ".LBB_" + m.group(1)
        if tgt in first and first[tgt] < hpos:
            inloop |= {x for x in order_all if first[tgt] <= first[x] < hpos}
mfma_loops = {inner_of[ins[i][2]] for i in mf if ins[i][2] in inner_of}


def in_inner(i):
    return inner_of.get(ins[i][2]) in mfma_loops


def kind(t):
    op = t.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("global_load") or op.startswith("buffer_load") or op.startswith("flat_load"):
        return "load"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op in ("s_waitcnt", "s_nop", "s_barrier", "s_sleep", "s_setprio") or op.startswith("s_sched"):
        return "wait"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return "other"


keys = ["valu", "salu", "branch", "execbr", "saveexec", "load", "lds", "mulhi"]
blocks, order = {}, []
for i, t, b in ins:
    if b not in inloop or in_inner(i):
        continue
    if b not in blocks:
        blocks[b] = dict.fromkeys(keys, 0)
        order.append(b)
    c = blocks[b]
    k = kind(t)
    if k in c:
        c[k] += 1
    op = t.split()[0]
    if op in ("s_cbranch_execz", "s_cbranch_execnz"):
        c["execbr"] += 1
    if "saveexec" in op:
        c["saveexec"] += 1
    # (the quotient step of an integer-division expansion; 64-bit products use it too)
    if op in ("s_mul_hi_u32", "v_mul_hi_u32"):
        c["mulhi"] += 1

percol = set(".LBB_" + x.split("_")[-1] for x in a.c.split(",") if x)
tot = {"tile": dict.fromkeys(keys, 0), "column": dict.fromkeys(keys, 0)}
for b in order:
    w = "column" if b in percol else "tile"
    for k in keys:
        tot[w][k] += blocks[b][k]
if a.v:
    print("block".ljust(12) + "".join(k.rjust(9) for k in keys))
    for b in order:
        print((b + ("*" if b in percol else "")).ljust(12) +
              "".join(str(blocks[b][k]).rjust(9) for k in keys))
print("kernel " + lines[start].split(":")[0])
print(f"tile loop (header BB_{H}): {sum(1 for i, t, b in ins if b in inloop)} instructions, "
      f"{len(mfma_loops)} MFMA loop(s)")
for h in sorted(mfma_loops, key=int):
    sel = [t for i, t, b in ins if inner_of.get(b) == h]
    c = {k: sum(1 for t in sel if kind(t) == k) for k in ("mfma", "valu", "salu", "lds")}
    print(f"  MFMA loop BB_{h}: {c['mfma']} MFMA, {c['valu']} VALU, {c['salu']} SALU, "
          f"{c['lds']} LDS per trip (static)")
nm = sum(1 for i in mf if ins[i][2] in inloop and not in_inner(i))
if nm:
    print(f"  MFMAs outside the MFMA loops: {nm}")
print("outside the MFMA loops  " + "".join(k.rjust(9) for k in keys))
for w in ("tile", "column"):
    print(f"  per {w}".ljust(24) + "".join(str(tot[w][k]).rjust(9) for k in keys))
