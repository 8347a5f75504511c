#!/usr/bin/env python3
"""Static instruction census of gfx950 kernels from a compiler listing (no GPU involved).

    hipcc <the Makefile's FLAGS> --cuda-device-only -S qmlp.hip -o qmlp.s
    tools/isa_census.py qmlp.s qact3p_kernelILi1E qact3h_kernelILb0ELi1ELb1E ...

For every kernel whose mangled name contains one of the given substrings it prints, as markdown,
the whole kernel, every loop that holds matrix instructions (a loop = a branch back to an earlier
label: from the target label to the branch), and the outermost such loop cut into the segments
between its workgroup barriers. Instructions are classified by mnemonic prefix only; every path is
counted once, so a census is a static figure, not a cycle count.

Besides the generic prefixes (v_mfma, v_, ds_, global_ / buffer_ / flat_, scratch_, s_) the table
splits off the sub-classes a spill and issue census needs, each again by prefix (CLASSES below):
32-bit integer multiplies, lane reads and writes (what SGPR spills compile to), packed f32 VALU,
waits and nops, barriers, scalar loads, branches. It looks for no other instruction.
"""
import argparse
import re
import sys

# first match wins
CLASSES = [
    ("mfma", ("v_mfma",)),
    ("imul", ("v_mul_lo", "v_mul_hi", "v_mad_u64", "v_mad_i64")),
    ("lane", ("v_readlane", "v_writelane", "v_readfirstlane")),
    ("pk_f32", ("v_pk_add_f32", "v_pk_mul_f32", "v_pk_fma_f32")),
    ("valu", ("v_",)),
    ("lds", ("ds_",)),
    ("vmem", ("global_", "buffer_", "flat_")),
    ("scratch", ("scratch_",)),
    ("wait", ("s_waitcnt", "s_nop", "s_sleep")),
    ("barrier", ("s_barrier",)),
    ("smem", ("s_load", "s_buffer_load")),
    ("branch", ("s_branch", "s_cbranch")),
    ("salu", ("s_",)),
]
COLS = [c for c, _ in CLASSES]
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")
TARGET = re.compile(r"(\.LBB\d+_\d+)")


def classify(mn):
    for name, prefixes in CLASSES:
        if mn.startswith(prefixes):
            return name
    return None


def kernel_bodies(path, wanted):
    """{symbol: [lines]} of every function whose symbol contains one of `wanted`."""
    out, cur, sym = {}, None, None
    with open(path) as f:
        for line in f:
            m = re.match(r"^(_Z\w+):", line)
            if m and cur is None:
                if any(w in m.group(1) for w in wanted):
                    sym, cur = m.group(1), []
                continue
            if cur is not None:
                if line.startswith(".Lfunc_end"):
                    out[sym] = cur
                    cur = None
                else:
                    cur.append(line.rstrip("\n"))
    return out


def parse(lines):
    """[(kind, text)]: kind 'label' (text = the label) or a class name (text = mnemonic + operands)"""
    items = []
    for ln in lines:
        m = LABEL.match(ln)
        if m:
            items.append(("label", m.group(1)))
            continue
        m = INSN.match(ln)
        if not m or ln.lstrip().startswith((";", ".")):
            continue
        c = classify(m.group(1))
        if c:
            items.append((c, m.group(1) + m.group(2)))
    return items


def count(items):
    n = dict.fromkeys(COLS, 0)
    for kind, _ in items:
        if kind != "label":
            n[kind] += 1
    return n


def loops(items):
    """(start, end) item index ranges of the back-edges, outermost first"""
    at = {text: i for i, (kind, text) in enumerate(items) if kind == "label"}
    found = []
    for i, (kind, text) in enumerate(items):
        if kind == "branch":
            m = TARGET.search(text)
            if m and m.group(1) in at and at[m.group(1)] < i:
                found.append((at[m.group(1)], i))
    widest = {}  # several branches back to one label: the loop is the widest of them
    for s, e in found:
        widest[s] = max(widest.get(s, e), e)
    return sorted(widest.items())


def row(name, n):
    return "| " + name + " | " + " | ".join(str(n[c]) for c in COLS) + " |"


def report(sym, items, out):
    head = "| part | " + " | ".join(COLS) + " |"
    out.write("### `%s`\n\n%s\n|%s\n" % (sym, head, "---|" * (len(COLS) + 1)))
    out.write(row("whole kernel", count(items)) + "\n")
    mf = [(s, e) for s, e in loops(items) if count(items[s:e + 1])["mfma"]]
    for s, e in mf:
        depth = sum(1 for s2, e2 in mf if s2 <= s and e <= e2 and (s2, e2) != (s, e))
        out.write(row("%sloop %s (%d instructions)" % ("&nbsp;&nbsp;" * depth, items[s][1], e - s), count(items[s:e + 1])) + "\n")
    if mf:
        s, e = max(mf, key=lambda r: r[1] - r[0])
        seg, k = [], 0
        for it in items[s:e + 1]:
            seg.append(it)
            if it[0] == "barrier":
                out.write(row("&nbsp;&nbsp;%s segment %d (to a barrier)" % (items[s][1], k), count(seg)) + "\n")
                seg, k = [], k + 1
        out.write(row("&nbsp;&nbsp;%s segment %d (to the back-edge)" % (items[s][1], k), count(seg)) + "\n")
    out.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("kernels", nargs="+", help="substrings of mangled kernel names")
    a = ap.parse_args()
    bodies = kernel_bodies(a.listing, a.kernels)
    if not bodies:
        sys.exit("no kernel matches")
    for sym in sorted(bodies):
        report(sym, parse(bodies[sym]), sys.stdout)


if __name__ == "__main__":
    main()
