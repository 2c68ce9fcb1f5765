#!/usr/bin/env python3
"""Static instruction account of one gfx950 kernel, phase by phase (no GPU involved).

    python scripts/step_isa_account.py TREE --kernel 'tiny_ecg_step_kernelILi16ELi4ELb0ELb1ELb1E' \
        [--file tiny_ecg_step.hip] [--path NAME=SEG:DECISIONS ...] [--trace]
    python scripts/step_isa_account.py --asm FILE.s --kernel SUBSTRING ...

``csrc/kernels/<file>`` of TREE is compiled device-only to assembly with the flags that tree's ``csrc/build.py`` uses
(the compile and the per-symbol split are ``scripts/diff_device_asm.py``'s).  The body of the one kernel whose symbol
contains ``--kernel`` is cut at its workgroup barriers: segment k is the code between barrier k - 1 and barrier k, which
for the TinyECG step kernels are the phases that ``ECG_STAMP`` marks (the bf16 kernels have no barrier between phase 0
and phase 1: their segment 0 is both, and segment k is phase k + 1).  Instructions are counted per segment by class,
and the class is the mnemonic's prefix, nothing else:

    mfma   v_mfma*            valu   every other v_*         lds   ds_*
    vmem   buffer_* global_*  salu   every s_*               other whatever is left

The static count of a segment is every instruction in its text.  What one wave issues is a path through it: ``--path
NAME=SEG:DECISIONS`` walks segment SEG from its first instruction and counts what lies on the way.  Every conditional
branch (``s_cbranch_*``) met on the walk takes the next character of DECISIONS: ``t`` the branch is taken, ``n`` it
falls through; when the string is used up, branches fall through.  ``s_branch`` is always followed, also to a block
that the compiler placed behind the last barrier, and the walk ends at the first barrier (or ``s_endpgm``) it
reaches.  ``--trace`` prints every decision with its line, which is how a
DECISIONS string is written and checked: a skipped ``s_cbranch_execz`` region is one whose exec mask is empty for that
wave (a thread range of ``row_store``), a taken ``s_cbranch_scc1`` in front of the head is a wave other than wave 0.
A walk counts a loop body once per time the decisions send it round.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import re
import sys
from typing import Dict, List, Optional, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("diff_device_asm", os.path.join(_HERE, "diff_device_asm.py"))
dda = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dda)

CLASSES = ["mfma", "valu", "lds", "vmem", "salu", "other"]
_LABEL = re.compile(r"^([.\w$]+):")
_MNEMONIC = re.compile(r"^[a-z][a-z0-9_]*$")


def classify(mnemonic: str) -> str:
    """The class of a mnemonic, by its prefix only."""
    if mnemonic.startswith("v_mfma"):
        return "mfma"
    if mnemonic.startswith("v_"):
        return "valu"
    if mnemonic.startswith("ds_"):
        return "lds"
    if mnemonic.startswith(("buffer_", "global_")):
        return "vmem"
    if mnemonic.startswith("s_"):
        return "salu"
    return "other"


Item = Tuple[str, str, str]  # ("label", name, "") or ("ins", mnemonic, operands)


def parse_body(lines: List[str]) -> List[Item]:
    """Labels and instructions of a kernel's lines, in order, up to the end of its code (the first directive that
    leaves the text section, or ``.Lfunc_end``); comments and directives are dropped."""
    items: List[Item] = []
    started = False
    for line in lines:
        s = line.split(";", 1)[0].strip()
        if not s:
            continue
        m = _LABEL.match(s)
        if m:
            if m.group(1).startswith(".Lfunc_end"):
                break
            items.append(("label", m.group(1), ""))
            started = True
            continue
        if s.startswith("."):
            if started and s.split()[0] in (".section", ".amdhsa_kernel"):
                break
            continue
        parts = s.split(None, 1)
        if started and _MNEMONIC.match(parts[0]):
            items.append(("ins", parts[0], parts[1] if len(parts) > 1 else ""))
    return items


def split_segments(items: List[Item]) -> List[List[Item]]:
    """The items cut behind every ``s_barrier`` (the barrier is the last instruction of the segment it ends)."""
    segs: List[List[Item]] = [[]]
    for it in items:
        segs[-1].append(it)
        if it[0] == "ins" and it[1] == "s_barrier":
            segs.append([])
    return segs


def count(items: List[Item]) -> Dict[str, int]:
    out = {c: 0 for c in CLASSES}
    for kind, mn, _ in items:
        if kind == "ins":
            out[classify(mn)] += 1
    return out


def walk(seg: List[Item], decisions: str, start: int = 0,
         max_steps: int = 100000) -> Tuple[Dict[str, int], List[str]]:
    """Counts along one path (module docstring) and the trace of its branch decisions.  ``seg`` is one segment, or
    the whole kernel with ``start`` at a segment's first item: the walk then follows branches to blocks that the
    compiler placed behind the kernel's last barrier, and ends at the first barrier it reaches."""
    where = {it[1]: i for i, it in enumerate(seg) if it[0] == "label"}
    out = {c: 0 for c in CLASSES}
    trace: List[str] = []
    i, d, steps = start, 0, 0
    while i < len(seg):
        steps += 1
        if steps > max_steps:
            raise RuntimeError("walk does not end: the decisions keep a loop running")
        kind, mn, ops = seg[i]
        i += 1
        if kind != "ins":
            continue
        out[classify(mn)] += 1
        if mn in ("s_endpgm", "s_barrier"):
            break
        target: Optional[str] = None
        if mn == "s_branch":
            target = ops.strip()
        elif mn.startswith("s_cbranch_"):
            ch = decisions[d] if d < len(decisions) else "n"
            if ch not in "tn":
                raise ValueError(f"decision {ch!r}: expected t or n")
            trace.append(f"{'#' + str(d) if d < len(decisions) else 'default':>8s} {ch}  {mn} {ops}")
            d += 1
            if ch == "t":
                target = ops.strip()
        if target is not None:
            if target not in where:
                trace.append(f"         leaves the segment at {target}")
                break
            i = where[target]
    return out, trace


def find_kernel(pieces: Dict[str, List[str]], needle: str) -> str:
    hits = [n for n in pieces if n != dda.OUTSIDE and needle in n]
    if len(hits) != 1:
        raise ValueError(f"--kernel {needle!r} matches {len(hits)} kernel symbols: {hits}")
    return hits[0]


def fmt_row(name: str, c: Dict[str, int]) -> str:
    return f"{name:<28s}" + "".join(f"{c[k]:>7d}" for k in CLASSES) + f"{sum(c.values()):>8d}"


def account(asm: str, needle: str, paths: List[str], trace: bool) -> List[str]:
    pieces = dda.split_kernels(asm)
    name = find_kernel(pieces, needle)
    segs = split_segments(parse_body(pieces[name]))
    out = [f"kernel {name}", f"{len(segs)} segments (cut behind each s_barrier)", "",
           f"{'static (all code)':<28s}" + "".join(f"{k:>7s}" for k in CLASSES) + f"{'all':>8s}"]
    total = {c: 0 for c in CLASSES}
    for k, seg in enumerate(segs):
        c = count(seg)
        out.append(fmt_row(f"  segment {k}", c))
        for key in CLASSES:
            total[key] += c[key]
    out.append(fmt_row("  whole kernel", total))
    if paths:
        out += ["", f"{'paths (one wave)':<28s}" + "".join(f"{k:>7s}" for k in CLASSES) + f"{'all':>8s}"]
    for spec in paths:
        pname, _, rest = spec.partition("=")
        seg_s, _, decisions = rest.partition(":")
        k = int(seg_s)
        c, tr = walk([it for seg in segs for it in seg], decisions, start=sum(len(seg) for seg in segs[:k]))
        out.append(fmt_row(f"  seg {seg_s} {pname}", c))
        if trace:
            out += [f"      {t}" for t in tr]
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tree", nargs="?", help="source tree to compile (omit with --asm)")
    ap.add_argument("--asm", help="an assembly file to read instead of compiling")
    ap.add_argument("--file", default="tiny_ecg_step.hip", help="kernel file under csrc/kernels/")
    ap.add_argument("--kernel", required=True, help="substring that picks one kernel symbol")
    ap.add_argument("--path", action="append", default=[], help="NAME=SEG:DECISIONS (t / n per conditional branch)")
    ap.add_argument("--trace", action="store_true", help="print every branch decision of every path")
    a = ap.parse_args(argv)
    if a.asm:
        with open(a.asm) as f:
            asm = f.read()
    elif a.tree:
        asm = dda.device_asm(os.path.abspath(a.tree), a.file)
    else:
        ap.error("give a TREE or --asm FILE")
    print("\n".join(account(asm, a.kernel, a.path, a.trace)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
