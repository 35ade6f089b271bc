#!/usr/bin/env python3
"""Lint for kernels whose global loads are inline asm with explicit vmcnt waits (conv_thin4_mfma_kernel, conv_bf3*_kernel,
wgrad_bf3_kernel, tools/ubench/wgrad1x1_direct.hip): hipcc does not know that the destination registers of an asm load are in
flight, so nothing stops it from reading (copying, spilling) or overwriting them before the matching asm wait -- the
register-allocation accidents DESIGN.md 3.6 / 3.11 describe, each of which gave wrong results on the GPU and clean code on
paper.  This follows the control flow of each kernel and keeps the queue of loads in flight: an asm `s_waitcnt vmcnt(N)` retires
all but the youngest N (vector memory operations return in order); compiler-issued vector memory instructions enter the queue
too (they count in vmcnt); a compiler-issued `s_waitcnt vmcnt(N)` retires likewise.  Every instruction outside an asm block that
reads or writes a register of an asm load still in the queue is reported, with the path by which the load reached it.

    python tools/isa_inflight_check.py <file.s> [kernel-name-substring ...]        exit code 1 if anything is reported

Control flow: the kernel is split into basic blocks (a label starts one; `s_branch`, `s_cbranch_*`, `s_setpc_b64` and
`s_endpgm` end one; a conditional branch and a block without a jump also fall through).  The queue at each block's entry is the
join of the queues its predecessors leave, iterated to a fixed point: aligned at the youngest entry, the longest queue, each
depth holding the union of the registers in flight there on any path -- the most conservative state, so a latch that copies a
register, a branch around an asm wait and a back edge that re-enters a loop header with a different queue than its prologue are
all seen.  The queue is capped at 63 entries (the hardware counter's limit: an older entry has returned before another issues),
which bounds the lattice; the iteration is bounded as well and a kernel that does not settle is reported as a finding."""
import re
import sys

REG = re.compile(r"\b([va])\[(\d+):(\d+)\]|\b([va])(\d+)\b")
VMEM = ("global_load", "global_store", "global_atomic", "buffer_", "flat_", "scratch_")
QMAX = 63                                             # vmcnt saturates at 63 outstanding operations on gfx9
LABEL = re.compile(r"^([.\w$]+):")


def regs_of(tok):
    out = set()
    for m in REG.finditer(tok):
        if m.group(1):
            out.update((m.group(1), r) for r in range(int(m.group(2)), int(m.group(3)) + 1))
        else:
            out.add((m.group(4), int(m.group(5))))
    return out


def _parse(lines):
    """-> list of blocks: dict(label, insns=[(line number, text, in_asm)], succ=[label or index], term)."""
    blocks = []
    cur = None
    in_asm = False

    def new(label):
        b = dict(label=label, insns=[], jumps=[], falls=True)
        blocks.append(b)
        return b

    for ln, raw in lines:
        if "#ASMSTART" in raw:
            in_asm = True
            continue
        if "#ASMEND" in raw:
            in_asm = False
            continue
        l = raw.split(";")[0].strip()
        m = LABEL.match(l)
        if m and not in_asm:
            cur = new(m.group(1))
            continue
        if not l or l.startswith("."):
            continue
        if cur is None:
            cur = new("<entry>")
        op = l.split()[0]
        cur["insns"].append((ln, l, in_asm))
        if in_asm:
            continue
        if op == "s_branch" or op.startswith("s_cbranch_"):
            cur["jumps"].append(l.split()[1])
            cur["falls"] = op != "s_branch"
            cur = new(None)
        elif op in ("s_endpgm", "s_setpc_b64"):
            cur["falls"] = False
            cur = new(None)
    blocks = [b for b in blocks if b["insns"] or b["label"] is not None]
    index = {b["label"]: i for i, b in enumerate(blocks) if b["label"] is not None}
    for i, b in enumerate(blocks):
        succ = [index[t] for t in b["jumps"] if t in index]
        if b["falls"] and i + 1 < len(blocks):
            succ.append(i + 1)
        b["succ"] = succ
    return blocks


def _step(queue, insn, found=None):
    """Apply one instruction to a queue (a tuple, oldest first, of frozensets of (asm destination register, line of its load);
    empty for a compiler-issued operation); report (line, text, registers hit, lines of the loads hit) into `found` if given."""
    ln, l, in_asm = insn
    op = l.split()[0]
    if op == "s_waitcnt":
        m = re.search(r"vmcnt\((\d+)\)", l)
        if m:
            n = int(m.group(1))
            queue = queue[len(queue) - n:] if 0 < n < len(queue) else (() if n == 0 else queue)
        return queue
    is_vmem = op.startswith(VMEM)
    if in_asm:
        if is_vmem and "load" in op and "_lds_" not in op:          # (LDS-DMA loads have no destination register)
            dst = l.split(None, 1)[1].split(",")[0]
            queue = queue + (frozenset((r, ln) for r in regs_of(dst)),)
        elif is_vmem:
            queue = queue + (frozenset(),)
        return queue[-QMAX:]
    if found is not None and queue:
        used = regs_of(l.split(None, 1)[1]) if " " in l else set()
        if used:
            hit = {(r, src) for q in queue for r, src in q if r in used}
            if hit:
                found.append((ln, l, sorted({r for r, _ in hit})[:4], sorted({src for _, src in hit})))
    if is_vmem:
        queue = queue + (frozenset(),)
    return queue[-QMAX:]


def _join(a, b):
    """Most conservative of two queues: aligned at the youngest entry, the longer length, the union at every depth."""
    if a is None:
        return b
    n = max(len(a), len(b))
    a = (frozenset(),) * (n - len(a)) + a
    b = (frozenset(),) * (n - len(b)) + b
    return tuple(x | y for x, y in zip(a, b))


def check_kernel(name, lines, max_rounds=200):
    """-> list of (line, instruction, registers hit, path) findings."""
    blocks = _parse(lines)
    if not blocks:
        return []
    nb = len(blocks)
    entry = [None] * nb                   # queue at block entry
    via = [dict() for _ in range(nb)]     # issuing line -> predecessor block that first brought it in
    entry[0] = ()
    work, rounds, settled = [0], 0, True
    while work:
        rounds += 1
        if rounds > max_rounds * nb:
            settled = False
            break
        i = work.pop(0)
        q = entry[i]
        for insn in blocks[i]["insns"]:
            q = _step(q, insn)
        for s in blocks[i]["succ"]:
            j = _join(entry[s], q)
            if j != entry[s]:
                for e in q:
                    for _, ln in e:
                        via[s].setdefault(ln, i)
                entry[s] = j
                if s not in work:
                    work.append(s)
    bad = []
    for i, b in enumerate(blocks):
        if entry[i] is None:
            continue                      # unreachable
        q, found = entry[i], []
        for insn in b["insns"]:
            q = _step(q, insn, found)
        for ln, l, hit, loads in found:
            bad.append((ln, l, hit, _path(blocks, via, i, loads[0], ln)))
    if not settled:
        bad.append((0, "<no fixed point>", [], f"the queue did not settle within {max_rounds} rounds per block"))
    return bad


def _name(blocks, i):
    return blocks[i]["label"] or f"<block after line {blocks[i - 1]['insns'][-1][0]}>" if i else (blocks[0]["label"] or "<entry>")


def _path(blocks, via, i, load_ln, use_ln):
    """The chain of blocks from the load at line load_ln to block i, back edges named."""
    def has(k):
        return any(x[0] == load_ln for x in blocks[k]["insns"])
    if has(i) and load_ln < use_ln:
        return f"load at line {load_ln}, same block"
    chain, k, seen = [i], i, set()            # (i itself may be the source: a loop of one block, or the way round a loop)
    while True:
        p = via[k].get(load_ln)
        if p is None or p in seen:
            break
        chain.append(p)
        seen.add(p)
        k = p
        if has(k):
            break
    chain.reverse()
    steps = []
    for a, b in zip(chain, chain[1:]):
        kind = "back edge" if b <= a else "edge"
        steps.append(f"{kind} {_name(blocks, a)} -> {_name(blocks, b)}")
    return f"load at line {load_ln}, via " + ", ".join(steps) if steps else f"load at line {load_ln}"


def main():
    path, pats = sys.argv[1], sys.argv[2:]
    txt = open(path).read().split("\n")
    starts = [i for i, l in enumerate(txt) if re.match(r"^[_A-Za-z][\w$.]*:\s*(;.*)?$", l) and not l.startswith(".L")]
    total = 0
    nker = 0
    for k, s in enumerate(starts):
        name = txt[s].split(":")[0]
        if pats and not any(p in name for p in pats):
            continue
        e = starts[k + 1] if k + 1 < len(starts) else len(txt)
        body = [(i + 1, txt[i]) for i in range(s + 1, e)]
        if not any("#ASMSTART" in b[1] for b in body):
            continue
        nker += 1
        bad = check_kernel(name, body)
        print(f"{name[:110]}: {len(bad)} instruction(s) touch a register with an asm load in flight")
        for ln, l, hit, via in bad[:8]:
            print(f"    line {ln}: {l}    <- {hit}  ({via})")
        total += len(bad)
    print(f"{nker} kernel(s) with asm blocks checked, {total} finding(s)")
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
