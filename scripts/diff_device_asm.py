#!/usr/bin/env python3
"""Compare the gfx950 device assembly of kernel files between two source trees, kernel by kernel.

    python scripts/diff_device_asm.py TREE_A TREE_B tiny_ecg_step.hip [tiny_ecg_eval.hip ...]
    python scripts/diff_device_asm.py TREE_A TREE_B tiny_ecg_step.hip=tiny_ecg_step.hip+tiny_ecg_close.hip

A bare file name is that file in both trees.  ``a.hip=b1.hip+b2.hip`` compares the kernels of TREE_A's ``a.hip`` with
the union of the kernels of TREE_B's ``b1.hip`` and ``b2.hip`` (``+`` works on either side) - for a refactor that moves
kernels between files.  A kernel defined by two files of one side is an error, and with several files on a side only
the kernels are compared, not what lies outside them.

Each ``csrc/kernels/<file>`` of each tree is compiled device-only to assembly with the flags that tree's
``csrc/build.py`` uses for it (``HIP_FLAGS`` + ``FILE_FLAGS[<file>]``, imported, not copied).  The text is split per
``.amdhsa_kernel`` symbol (a kernel's code and its kernel descriptor), the ``__hip_cuid_<hash>`` symbol - a hash of
the source text - is ignored, and every kernel is reported as identical or with its first differing lines.  Whatever
lies outside the kernels (metadata, other functions) is compared as one more piece.  Exit status 1 on any difference
or when the two builds do not define the same kernel symbols.  A refactor that claims "same machine code" proves it
with this; the tool compares text and knows nothing about instructions.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from typing import Dict, List, Tuple

OUTSIDE = "(outside kernels)"
_CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
# A function's local labels carry its ordinal in the file (.LBB20_3, .Lfunc_end20): the order in which hipcc emits the
# functions - for templates, the order of their first uses - and no part of the code.  (The loop comments name blocks
# without the ".L": "Header=BB20_16".)
_FN_ORDINAL = re.compile(r"\b(LBB|BB|LJTI|Lfunc_begin|Lfunc_end)\d+")
_RESOURCE = re.compile(r"\.set\s+(\S+)\.(?:num_vgpr|num_agpr|numbered_sgpr|num_named_barrier|private_seg_size|uses_vcc|"
                       r"uses_flat_scratch|has_dyn_sized_stack|has_recursion|has_indirect_call)\s*,")
_COMMENT_PAD = re.compile(r"[ \t]+;")
_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")


def split_kernels(asm: str) -> Dict[str, List[str]]:
    """``{kernel symbol: lines, OUTSIDE: every other line}`` of one assembly file.  A kernel's lines run from its
    label ``<sym>:`` to its ``.size <sym>, ...`` directive (hipcc puts the ``.amdhsa_kernel <sym>`` ..
    ``.end_amdhsa_kernel`` descriptor inside that range; one that stands alone is added to its kernel too), plus the
    ``.set <sym>.num_vgpr, ...`` lines of its register and scratch figures, which hipcc puts behind ``.size``.
    ``__hip_cuid_<hash>`` is replaced by ``__hip_cuid_`` everywhere, and local labels lose their function's ordinal in
    the file (``.LBB20_3`` -> ``.LBB_3``), which follows the order of the functions, not their code."""
    text = _FN_ORDINAL.sub(r"\1", _CUID.sub("__hip_cuid_", asm))
    lines = _COMMENT_PAD.sub(" ;", text).splitlines()  # a label's length sets the column of the comment behind it
    names = [m.group(1) for m in map(_KERNEL.match, lines) if m]
    pieces: Dict[str, List[str]] = {n: [] for n in names}
    pieces[OUTSIDE] = []
    cur = None  # the kernel whose code or descriptor the current line belongs to
    in_code = False  # between the label and .size (hipcc emits the descriptor inside that range)
    for line in lines:
        s = line.split(";", 1)[0].strip()  # without the trailing comment
        m = _KERNEL.match(line)
        if cur is None and m:
            cur = m.group(1)
        elif cur is None and s.endswith(":") and s[:-1] in names:
            cur, in_code = s[:-1], True
        res = _RESOURCE.match(s) if cur is None else None  # behind .size: the kernel's register and scratch figures
        if res and res.group(1) in pieces:
            pieces[res.group(1)].append(line)
            continue
        pieces[cur if cur is not None else OUTSIDE].append(line)
        if cur is not None and (s.split()[:2] == [".size", cur + ","] if in_code else s == ".end_amdhsa_kernel"):
            cur, in_code = None, False
    return pieces


def union_kernels(asms: List[str]) -> Dict[str, List[str]]:
    """The kernels of several assembly files of one tree as one ``{kernel symbol: lines}``; a single file keeps its
    ``OUTSIDE`` piece, several have none to compare.  ValueError when two files define the same kernel."""
    if len(asms) == 1:
        return split_kernels(asms[0])
    out: Dict[str, List[str]] = {}
    for asm in asms:
        for name, lines in split_kernels(asm).items():
            if name == OUTSIDE:
                continue
            if name in out:
                raise ValueError(f"kernel {name} is defined by more than one file of a tree")
            out[name] = lines
    return out


def compare(asm_a, asm_b, context: int = 3) -> Tuple[bool, List[str]]:
    """(everything identical, report lines) for two assembly texts, or two lists of texts (``union_kernels``)."""
    a, b = (union_kernels([t] if isinstance(t, str) else list(t)) for t in (asm_a, asm_b))
    if (OUTSIDE in a) != (OUTSIDE in b):  # one file against several: kernels only
        a.pop(OUTSIDE, None), b.pop(OUTSIDE, None)
    ok, report = True, []
    for name in sorted(set(a) - set(b)):
        ok = False
        report.append(f"MISSING in B   {name}")
    for name in sorted(set(b) - set(a)):
        ok = False
        report.append(f"MISSING in A   {name}")
    for name in [n for n in a if n in b]:
        la, lb = a[name], b[name]
        if la == lb:
            report.append(f"identical      {name}  ({len(la)} lines)")
            continue
        ok = False
        i = next((k for k, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
        report.append(f"DIFFERENT      {name}  (A {len(la)} lines, B {len(lb)} lines; first difference at line {i + 1})")
        report += [f"    A| {x}" for x in la[i:i + context]] + [f"    B| {x}" for x in lb[i:i + context]]
    return ok, report


def _build_module(tree: str):
    spec = importlib.util.spec_from_file_location(f"_build_{abs(hash(tree))}", os.path.join(tree, "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_asm(tree: str, fname: str) -> str:
    """``csrc/kernels/<fname>`` of ``tree`` compiled device-only to assembly with that tree's build flags."""
    b = _build_module(tree)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, fname + ".s")
        cmd = [b.hipcc(), *b.HIP_FLAGS, *b.FILE_FLAGS.get(fname, []), "-I", os.path.join(tree, "csrc", "include"),
               "--cuda-device-only", "-S", os.path.join(tree, "csrc", "kernels", fname), "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"compile failed: {' '.join(cmd)}\n{r.stdout}")
        with open(out) as f:
            return f.read()


def parse_spec(spec: str) -> Tuple[List[str], List[str]]:
    """``a.hip`` -> (["a.hip"], ["a.hip"]); ``a.hip=b1.hip+b2.hip`` -> (["a.hip"], ["b1.hip", "b2.hip"])."""
    side_a, _, side_b = spec.partition("=")
    return side_a.split("+"), (side_b or side_a).split("+")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("files", nargs="+", help="kernel file names under csrc/kernels/, or A.hip=B1.hip+B2.hip")
    a = ap.parse_args(argv)
    all_ok = True
    for spec in a.files:
        files_a, files_b = parse_spec(spec)
        asm_a = [device_asm(os.path.abspath(a.tree_a), f) for f in files_a]
        asm_b = [device_asm(os.path.abspath(a.tree_b), f) for f in files_b]
        ok, report = compare(asm_a, asm_b)
        all_ok &= ok
        lines_a, lines_b = (sum(len(t.splitlines()) for t in asm) for asm in (asm_a, asm_b))
        print(f"== {spec}: A {lines_a} lines, B {lines_b} lines")
        print("\n".join(report))
        print(f"== {spec}: {'all identical' if ok else 'DIFFERENCES'}")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
