#!/usr/bin/env python3
"""Per-kernel instruction-stream comparison of two builds of one object (a refactor's "what did the compiler make of it").

    llvm-objdump --offloading a/gemm.o && llvm-objdump -d a/gemm.o.0.hipv4-amdgcn-amd-amdhsa--gfx950 > a.txt   (same for b)
    tools/probes/isa_diff.py [--opcodes] a.txt b.txt

Every run prints three tallies for the object: kernels with an identical instruction stream, with an identical MNEMONIC stream (the same
instructions in the same order, operands aside: a commuted operand pair or another register assignment) and with equal length.  --opcodes
compares mnemonics only: kernels that differ in operands alone are not listed.

Addresses and encodings are stripped (branch operands are relative, so the text is position-independent).  A kernel whose stream differs
gets two rows of counts, before and after: instructions, then VMEM / DS / MFMA / s_waitcnt / barrier of the whole kernel and of its K-loop
bodies (every backward-branch range that holds an MFMA; nested ranges are counted once).

Assumes llvm-objdump's gfx9 syntax: a branch operand is the unsigned 16-bit word offset from the next instruction, so >= 32768 is a backward
branch.  A loop the compiler peels or duplicates is counted once per copy, so the K-loop columns compare the SUM over copies: when only those
columns differ and the whole-kernel columns agree, look at the loop structure before concluding anything.
"""
import re
import sys


def kernels(path):
    out, name = {}, None
    for ln in open(path):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", ln)
        if m and name:
            out[name].append((int(m.group(2), 16), re.sub(r"\s+", " ", m.group(1))))
    return out


def kind(ins):
    op = ins.split()[0]
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")): return "vmem"
    if op.startswith("ds_"): return "ds"
    if "mfma" in op: return "mfma"
    if op == "s_waitcnt": return "wait"
    if op == "s_barrier": return "bar"
    return None


def counts(body):
    c = dict.fromkeys(("vmem", "ds", "mfma", "wait", "bar"), 0)
    for _, ins in body:
        k = kind(ins)
        if k: c[k] += 1
    return c


def loop_body(body):
    """instructions inside backward-branch ranges that contain an MFMA"""
    inside = set()
    for i, (addr, ins) in enumerate(body):
        m = re.match(r"s_cbranch_\w+ (\d+)|s_branch (\d+)", ins)
        if not m: continue
        off = int(m.group(1) or m.group(2))
        if off < 32768: continue  # forward
        tgt = addr + 4 + (off - 65536) * 4
        rng = [j for j in range(i + 1) if body[j][0] >= tgt]
        if any(kind(body[j][1]) == "mfma" for j in rng): inside.update(rng)
    return [body[j] for j in sorted(inside)]


def row(body):
    w, l = counts(body), counts(loop_body(body))
    return "%6d | %s | %s" % (len(body), " ".join("%4d" % w[k] for k in w), " ".join("%4d" % l[k] for k in l))


def stream(body, opcodes):
    return [i.split()[0] if opcodes else i for _, i in body]


def main():
    args = [x for x in sys.argv[1:] if x != "--opcodes"]
    opcodes = len(args) != len(sys.argv) - 1
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = kernels(args[0]), kernels(args[1])
    if sorted(a) != sorted(b):
        print("KERNEL SETS DIFFER:", sorted(set(a) ^ set(b)))
    both = [k for k in a if k in b]
    ident = [k for k in both if stream(a[k], False) == stream(b[k], False)]
    mnem = [k for k in both if stream(a[k], True) == stream(b[k], True)]
    print("%d kernels, %d with an identical instruction stream, %d with an identical mnemonic stream, %d of equal length"
          % (len(a), len(ident), len(mnem), sum(len(a[k]) == len(b[k]) for k in both)))
    same = mnem if opcodes else ident
    print("differing kernels:  insns | whole kernel: vmem ds mfma wait bar | K-loop bodies: vmem ds mfma wait bar")
    for k in sorted(a):
        if k in b and k not in same:
            ra, rb = row(a[k]), row(b[k])
            flag = "" if ra.split("|")[1:] == rb.split("|")[1:] else "   <-- COUNTS DIFFER"
            print(k[:120])
            print("   before %s\n   after  %s%s" % (ra, rb, flag))


if __name__ == "__main__":
    main()
