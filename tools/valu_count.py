"""Static instruction count of a kernel's Newton loop in a gfx950 device .s (-save-temps).

The one-wave SCHUR fast pass is bound by the number of VALU instructions it issues
(DESIGN.md §4), so the count of its Newton step is a budget the build can be held to
without a GPU (tests/test_valu_budget.py).

The Newton loop is found from the control flow alone: every backward branch
(`s_cbranch_* / s_branch` to a label that precedes it) closes a loop that spans the
label .. the branch; the Newton loop is the smallest such span that holds a matrix-core
instruction (the Schur formation sits in no deeper loop of the SCHUR kernels).  Kernels
without MFMA take the largest span that is nested in another loop (the inner `while` of
the two-level continuation), or the largest span if there is only one level.

Every instruction in the span is counted once, by mnemonic prefix only:

    valu   v_*  except v_mfma_* / v_smfmac_*      mfma   v_mfma_* / v_smfmac_*
    lds    ds_*                                   vmem   global_* / flat_* / buffer_* / scratch_*
    salu   s_*  except s_waitcnt* / s_nop / s_barrier / branches
    wait   s_waitcnt* / s_nop / s_barrier         branch s_branch / s_cbranch_* / s_setpc / s_endpgm

`scratch` (scratch_* and buffer_* with `offen`/`off` on the scratch descriptor s[0:3]) is
reported beside vmem: a spill inside the loop.  The kernel's VGPR count comes from its
`.amdhsa_next_free_vgpr` / `; NumVgprs:` lines.

    python tools/valu_count.py file.s KERNEL-SUBSTRING [--json]
"""

from __future__ import annotations

import json
import re
import sys

CLASSES = ("valu", "mfma", "lds", "vmem", "salu", "wait", "branch", "other")


def classify(op: str) -> str:
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep")):
        return "wait"
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_endpgm", "s_swappc")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    return "other"


def is_scratch(text: str) -> bool:
    op = text.split()[0]
    return op.startswith("scratch_") or (op.startswith("buffer_") and "s[0:3]" in text)


def kernel_body(path: str, want: str):
    """(mangled name, [(text, label or None)], {resource comments}) of the first kernel whose name holds `want`."""
    name, body, meta, done = None, [], {}, False
    for l in open(path).read().split("\n"):
        t = l.split(";")[0].strip()
        if name is None:
            if t.endswith(":") and not t.startswith(".") and want in t:
                name = t[:-1]
            continue
        if t.startswith(".Lfunc_end"):
            done = True  # the kernel's text is over; its resource comments follow
        if done:
            m = re.match(r";\s*(NumVgprs|NumAgprs|ScratchSize|Occupancy):\s*(\d+)", l.strip())
            if m:
                meta[m.group(1)] = int(m.group(2))
                if m.group(1) == "Occupancy":
                    break
            continue
        if t.endswith(":") and t.startswith(".LBB"):
            body.append((None, t[:-1]))
        elif t and not t.startswith(".") and not t.endswith(":"):
            body.append((t, None))
    return name, body, meta


def blocks(body):
    """Basic blocks [(label or None, [instruction text])] and their successor lists."""
    blk, cur = [], (None, [])
    for t, lab in body:
        if lab is not None:
            if cur[1] or cur[0] is not None:
                blk.append(cur)
            cur = (lab, [])
            continue
        cur[1].append(t)
        if classify(t.split()[0]) == "branch":
            blk.append(cur)
            cur = (None, [])
    if cur[1] or cur[0] is not None:
        blk.append(cur)
    at = {lab: i for i, (lab, _) in enumerate(blk) if lab is not None}
    succ = []
    for i, (lab, ins) in enumerate(blk):
        s, last = [], (ins[-1].split() if ins else ["-"])
        if last[0].startswith(("s_cbranch", "s_branch")) and last[-1] in at:
            s.append(at[last[-1]])
        if not last[0].startswith(("s_branch", "s_endpgm", "s_setpc")) and i + 1 < len(blk):
            s.append(i + 1)
        succ.append(s)
    return blk, succ


def natural_loops(blk, succ):
    """Block sets {header} ∪ {blocks that reach the edge's tail without passing the header}, one per
    edge tail → header whose set stays clear of the entry block (i.e. per back edge)."""
    pred = [[] for _ in blk]
    for i, s in enumerate(succ):
        for j in s:
            pred[j].append(i)
    out = []
    for tail, s in enumerate(succ):
        for head in s:
            seen, todo = {head}, [tail]
            while todo:
                b = todo.pop()
                if b in seen:
                    continue
                seen.add(b)
                todo += pred[b]
            if 0 not in seen or head == 0:
                out.append((head, seen))
    return out


def newton_loop(blk, succ):
    size = lambda L: sum(len(blk[b][1]) for b in L[1])
    mfma = lambda L: any(classify(t.split()[0]) == "mfma" for b in L[1] for t in blk[b][1])
    ls = natural_loops(blk, succ)
    if not ls:
        return None
    with_mfma = [L for L in ls if mfma(L)]
    if with_mfma:
        return min(with_mfma, key=size)
    nested = [L for L in ls if any(o is not L and L[1] < o[1] for o in ls)]
    return max(nested or ls, key=size)


def count(path: str, want: str) -> dict:
    name, body, meta = kernel_body(path, want)
    if name is None:
        raise SystemExit(f"no kernel matching {want!r} in {path}")
    blk, succ = blocks(body)
    loop = newton_loop(blk, succ)
    if loop is None:
        raise SystemExit(f"{name}: no loop found")
    c = dict.fromkeys(CLASSES, 0)
    scratch = 0
    for b in sorted(loop[1]):
        for t in blk[b][1]:
            c[classify(t.split()[0])] += 1
            scratch += is_scratch(t)
    return {"kernel": name, "loop": blk[loop[0]][0], "blocks": len(loop[1]), "instructions": sum(c.values()), **c,
            "scratch_in_loop": scratch, "vgprs": meta.get("NumVgprs"), "agprs": meta.get("NumAgprs"),
            "scratch_bytes": meta.get("ScratchSize"), "occupancy": meta.get("Occupancy")}


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    as_json = "--json" in argv
    argv = [a for a in argv if a != "--json"]
    if len(argv) != 2:
        print(__doc__)
        return 2
    r = count(argv[0], argv[1])
    if as_json:
        print(json.dumps(r))
    else:
        print(f"{r['kernel']}\n  Newton loop at {r['loop']}: {r['instructions']} instructions")
        print("  " + "  ".join(f"{k} {r[k]}" for k in CLASSES))
        print(f"  scratch in loop {r['scratch_in_loop']}  VGPRs {r['vgprs']}  AGPRs {r['agprs']}  "
              f"scratch bytes {r['scratch_bytes']}  occupancy {r['occupancy']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
