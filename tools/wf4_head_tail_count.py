#!/usr/bin/env python
"""Instruction counts of conv_wf4_kernel instantiations by part -- head (up to the K loop), K loop body, tail (after it) --
out of gfx950 assembly (no GPU needed):

    hipcc -x hip <the flags of planer_amd/_build.py> --cuda-device-only -S planer_amd/csrc/conv_winograd.hip -o wino.s
    python tools/wf4_head_tail_count.py wino.s [mangled-name regex = the two shipped instantiations]

The K loop is the outermost loop that holds MFMAs; MFMAs in front of it (a peeled first step) count as head.  Static counts:
the tail holds all four variants of the output rows, of which a launch runs one (see profiles/wf4_head_tail.md).
"""
import re
import sys

CLASSES = ["mfma", "pk_f32", "v_mov", "valu", "lds", "vmem", "lds-dma", "scratch", "salu", "waitcnt", "branch", "barrier"]


def classify(text):
    op = text.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_pk_") and "f32" in op:
        return "pk_f32"
    if op.startswith("v_mov_b"):              # (the accumulator clear is 143 copies of one zeroed register)
        return "v_mov"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith(("buffer_", "global_", "flat_")):
        return "lds-dma" if re.search(r"\blds\b", text) else "vmem"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_barrier"):
        return "barrier"
    if op.startswith("s_"):
        return "salu"
    return None


def kernels(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w*conv_wf4_kernel\w*):", line)
        if m:
            name, body = m.group(1), []
        elif name:
            body.append(line.rstrip("\n"))
            if line.strip().startswith("s_endpgm"):
                yield name, body
                name = None


def parts(body):
    """-> (head, loop, tail) lists of instruction texts"""
    insts = []          # (text, label or None)
    for line in body:
        s = line.split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            insts.append((None, m.group(1)))
        elif s and not s.startswith(".") and not s.endswith(":"):
            insts.append((s, None))
    label_at = {lab: i for i, (t, lab) in enumerate(insts) if lab}
    # the K loop: the loop header with MFMAs between it and the LAST branch back to it (a rotated loop has several)
    best = None
    for i, (t, lab) in enumerate(insts):
        if t and t.startswith(("s_cbranch", "s_branch")):
            j = label_at.get(t.split()[-1])
            if j is not None and j < i and any(x and x.startswith("v_mfma") for x, _ in insts[j:i]):
                if best is None or j < best[0] or (j == best[0] and i > best[1]):
                    best = (j, i)
    if best is None:
        raise SystemExit("no loop with MFMAs")
    txt = lambda seg: [t for t, _ in seg if t]
    return txt(insts[:best[0]]), txt(insts[best[0]:best[1] + 1]), txt(insts[best[1] + 1:]), insts[best[1] + 1:]


def runs_with_stores(tail):
    """the tail's straight-line runs (no label, no branch inside) that hold 16-byte stores: (first instruction index, texts)"""
    run, start, k = [], 0, 0
    for t, lab in tail:
        if t:
            k += 1
        if lab or (t and t.startswith(("s_cbranch", "s_branch", "s_endpgm"))):
            if sum(x.startswith("buffer_store_dwordx4") for x in run) > 0:
                yield start, run
            run, start = [], k
        elif t:
            run.append(t)


def main():
    path = sys.argv[1]
    pat = sys.argv[2] if len(sys.argv) > 2 else r"ILi4ELb1ELb1ELb1E|ILi3ELb0ELb1ELb1E"
    for name, body in kernels(path):
        if not re.search(pat, name):
            continue
        print("## %s" % name)
        print("| part | total | " + " | ".join(CLASSES) + " |")
        print("|---|" + "---|" * (len(CLASSES) + 1))
        head, loop, tail, tail_raw = parts(body)
        rows = [("head", head), ("K loop body", loop), ("tail, all variants", tail)]
        rows += [("tail run at %d: %d stores" % (at, sum(x.startswith("buffer_store_dwordx4") for x in run)), run)
                 for at, run in runs_with_stores(tail_raw)]
        for part, seg in rows:
            n = dict.fromkeys(CLASSES, 0)
            for t in seg:
                c = classify(t)
                if c:
                    n[c] += 1
            print("| %s | %d | " % (part, sum(n.values())) + " | ".join(str(n[c]) for c in CLASSES) + " |")
        print()


if __name__ == "__main__":
    main()
