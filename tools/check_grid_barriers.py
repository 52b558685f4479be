#!/usr/bin/env python3
"""Post-build check of the hand-rolled grid barriers in libdlsa_hip.so (lars_c.hip, lars_q.hip, lars.hip's grid kernel in both
builds, irls_small.hip's cluster kernel).

Each barrier publishes what the workgroup wrote to global memory with ONE arrival: thread 0 releases at agent scope
(buffer_wbl2 + s_waitcnt vmcnt(0)) and adds to the counter.  That release orders only thread 0's own wave's stores: vmcnt counts
per wave, and __syncthreads() is a workgroup-scope fence that drains LDS (lgkmcnt) but not the vector memory counter.  So every
wave must itself wait for its global stores (s_waitcnt vmcnt(0): they are then in the XCD's L2, which thread 0's write-back
covers) BEFORE the workgroup barrier that thread 0 passes on its way to the arrival.  On the disassembly of the shipped code objects this
script finds every arrival -- an s_barrier, then buffer_wbl2, then global_atomic_add within a few instructions -- and requires that
no path of the kernel's control-flow graph leads from a global store to that s_barrier without passing an s_waitcnt with
vmcnt(0) (the compiler drops the fence's wait where its own count says nothing can be outstanding).
Run by tests/test_build_cpu.py.  Needs llvm-objcopy / llvm-readelf / llvm-objdump (ROCm's llvm/bin).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from check_agpr_kernels import code_objects, tool  # noqa: E402

# kernel (mangled name pattern) -> the fewest grid arrivals its source has (barrier call sites after inlining; a loose lower
# bound so that the check cannot pass on a kernel whose barriers it failed to recognise)
KERNELS = {
    r"lars_c_kernel": 4,
    r"lars_q_kernelILi\d+ELb0E": 3,           # (the LDS-resident builds, LDSQ = true, run on one workgroup: no barrier)
    r"lars_t1024\d+lars_grid_kernel": 6,
    r"lars_t512\d+lars_grid_kernel": 6,
    r"irls_small_kernelILi\d+E": 1,
}
WINDOW = 24          # instructions from the s_barrier to the arrival's atomic
BRANCHES = ("s_branch", "s_endpgm", "s_setpc_b64", "s_getpc_b64", "s_swappc_b64")
STORES = ("global_store", "global_atomic", "buffer_store", "buffer_atomic", "flat_store", "flat_atomic")


def disassemble(co):
    """name -> [(addr, mnemonic, operand text, branch target address or None)]"""
    txt = subprocess.check_output([tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    kern, name, start = {}, None, 0
    for ln in txt.splitlines():
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", ln)
        if m:
            name, start = m.group(2), int(m.group(1), 16)
            kern[name] = []
            continue
        m = re.match(r"^\s+(\S+)(.*?)//\s*([0-9A-Fa-f]+):", ln)
        if not m or name is None:
            continue
        op, rest, addr = m.group(1), m.group(2), int(m.group(3), 16)
        tgt = None
        if op.startswith("s_cbranch") or op == "s_branch":
            t = re.search(r"<%s\+0x([0-9a-f]+)>" % re.escape(name), ln)
            tgt = start + int(t.group(1), 16) if t else (start if ("<%s>" % name) in ln else None)
        kern[name].append((addr, op, rest.strip(), tgt))
    return kern


def arrivals(ins):
    """[(index of the s_barrier, index of the global_atomic_add, index of a store that can be outstanding at the barrier or None)]"""
    preds = predecessors(ins)
    out = []
    for i, (_, op, _, _) in enumerate(ins):
        if not op.startswith("global_atomic_add"):
            continue
        wb = bar = None
        for j in range(i - 1, max(-1, i - WINDOW), -1):
            o = ins[j][1]
            if o.startswith("global_atomic"):
                break
            if wb is None and o.startswith("buffer_wbl2"):
                wb = j
            elif wb is not None and o == "s_barrier":
                bar = j
                break
        if bar is None:
            continue
        out.append((bar, i, undrained_store(ins, preds, bar)))
    return out


def predecessors(ins):
    """instruction index -> indices of the instructions that can run just before it (fall-through and branches)"""
    index = {a: k for k, (a, _, _, _) in enumerate(ins)}
    preds = [[k - 1] if k and ins[k - 1][1] not in BRANCHES else [] for k in range(len(ins))]
    for k, (_, _, _, tgt) in enumerate(ins):
        if tgt in index:
            preds[index[tgt]].append(k)
    return preds


def undrained_store(ins, preds, bar):
    """index of a global store that can still be outstanding at the s_barrier `bar` (a path of the control-flow graph from the
    store to the barrier passes no s_waitcnt vmcnt(0)), or None"""
    stack, seen = list(preds[bar]), set()
    while stack:
        j = stack.pop()
        if j in seen:
            continue
        seen.add(j)
        _, o, rest, _ = ins[j]
        if o == "s_waitcnt" and re.search(r"\bvmcnt\(0\)", rest):
            continue
        if o.startswith(STORES):
            return j
        stack.extend(preds[j])
    return None


def check(lib=None, verbose=False):
    """(arrivals found per kernel pattern, problems): a problem names the kernel and the s_barrier's address"""
    lib = lib or os.path.join(ROOT, "dlsa_amd", "libdlsa_hip.so")
    found = {k: 0 for k in KERNELS}
    per_kernel, problems = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            for name, ins in disassemble(co).items():
                pats = [p for p in KERNELS if re.search(p, name)]
                if not pats:
                    continue
                arr = arrivals(ins)
                per_kernel[name] = (pats[0], len(arr))
                for bar, at, st in arr:
                    if st is not None:
                        problems.append((name, "arrival at 0x%x: the %s at 0x%x reaches its s_barrier (0x%x) with no s_waitcnt vmcnt(0)"
                                         % (ins[at][0], ins[st][1], ins[st][0], ins[bar][0])))
                if verbose:
                    print("%-64s %2d arrivals, %d with a store not waited for before the barrier" % (
                        name[:64], len(arr), sum(1 for a in arr if a[2] is not None)))
    for name, (pat, n) in per_kernel.items():
        found[pat] += 1
        if n < KERNELS[pat]:
            problems.append((name, "only %d grid arrivals recognised (at least %d expected)" % (n, KERNELS[pat])))
    for pat, n in found.items():
        if n == 0:
            problems.append((pat, "no such kernel in the library"))
    return per_kernel, problems


if __name__ == "__main__":
    kernels, bad = check(sys.argv[1] if len(sys.argv) > 1 else None, verbose=True)
    print("%d grid-barrier kernels checked, %d problems" % (len(kernels), len(bad)))
    for k, err in bad:
        print("  %s: %s" % (k, err))
    sys.exit(1 if bad or not kernels else 0)
