#!/usr/bin/env python
"""Static instruction counts of the segment kernel's worker loop, phase by phase (no GPU needed).

The worker loop of k3_segment (csrc/stage3.hpp) reads the shader clock at every K3_STAMP: an `s_memtime` whose value the next
`global_store_dwordx2 ... offset:<8 * slot>` puts into the stamp buffer.  This tool takes the device assembly of an inst3 unit
(`hipcc -S --cuda-device-only` with the Makefile's flags of the unit), finds one kernel in it, cuts the kernel's text at those clock reads
and counts the instructions between two consecutive ones by mnemonic prefix.  The α = 1, two-hand-over, one-handle, one-chunk kernel has two
units (csrc/stage3.hpp SMCMI_K3_RUN), told apart by the name prefix:

  _ZN5smcmi10k3_segmentILi10ELb1ELb0E         the general unit (inst3g_d10: -DSMCMI_INST3_D=10 -DSMCMI_INST3_A=1 -DSMCMI_INST3_R=0)
  _ZN5smcmi6defrun10k3_segmentILi10ELb1ELb0E  the default-run unit (inst3_d10: the same with -DSMCMI_INST3_U=1) - it has no stamps to cut at
                                              unless it is compiled with -DSMCMI_K3_KEEP=1 (the development build: VARIANT_FLAGS)

Columns:

  valu     every v_* instruction
  select   v_cndmask*
  mov      v_mov* / v_accvgpr* without a DPP modifier (register copies)
  xlane    DPP forms, v_permlane*, v_readlane*, v_readfirstlane*, v_writelane*, ds_bpermute*, ds_swizzle* (data crossing lanes)
  reload   v_readlane_b32 out of a spill VGPR - a VGPR that the kernel writes with v_writelane_b32 (the compiler's home for spilled scalars)
  s_nop    s_nop
  fp64     v_add_f64, v_mul_f64, v_fma_f64

The text is cut in layout order, which for this kernel is program order; a rarely taken branch laid out between two stamps counts in that
phase.  Counts are static: a loop body counts once.  A counting aid - it checks nothing.

--blocks FROM TO prints the census of ONE phase (the text between the stamps of slots FROM and TO) per basic block - the text between two
labels - with the columns above and two more:

  lds_read ds_read*
  div      v_div_fixup* (one per division the compiler expanded)

so that a block such as the MH step's bounds check + log-prior can be read off without a script of one's own.

usage: python tools/phase_isa.py <device.s> <mangled kernel name prefix> [--json] [--blocks FROM TO]"""
import json
import re
import sys

COLUMNS = ("valu", "select", "mov", "xlane", "reload", "s_nop", "fp64")
_XLANE = ("v_permlane", "v_readlane", "v_readfirstlane", "v_writelane", "ds_bpermute", "ds_swizzle")
_FP64 = ("v_add_f64", "v_mul_f64", "v_fma_f64")
_STAMP_REACH = 16        # lines behind an s_memtime within which its store is looked for


def kernel_text(asm, prefix):
    """The lines of the first function whose label starts with `prefix`, label and end marker excluded."""
    lines = asm.split("\n")
    start = next((i for i, ln in enumerate(lines) if ln.startswith(prefix) and ln.split(";")[0].rstrip().endswith(":")), None)
    if start is None:
        raise ValueError("no kernel whose name starts with %r" % prefix)
    out = []
    for ln in lines[start + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        out.append(ln)
    return out


def _instruction(line):
    """(mnemonic, operand text) of an assembly line, or None for labels, directives, comments and blank lines."""
    t = line.split(";")[0].strip()
    if not t or t.startswith(".") or t.endswith(":"):
        return None
    parts = t.split(None, 1)
    return parts[0], (parts[1] if len(parts) > 1 else "")


def spill_vgprs(lines):
    """The VGPRs the kernel keeps spilled scalars in: every destination of a v_writelane_b32."""
    regs = set()
    for ln in lines:
        ins = _instruction(ln)
        if ins and ins[0].startswith("v_writelane_b32"):
            regs.add(ins[1].split(",")[0].strip())
    return regs


def classify(op, args, spills):
    """The columns an instruction counts in."""
    cols = []
    dpp = "_dpp" in op or "row_" in args or "quad_perm" in args or "wave_" in args or "bank_mask" in args
    if op.startswith("v_"):
        cols.append("valu")
    if op.startswith("v_cndmask"):
        cols.append("select")
    if op.startswith(("v_mov", "v_accvgpr")) and not dpp:
        cols.append("mov")
    if dpp or op.startswith(_XLANE):
        cols.append("xlane")
    if op.startswith("v_readlane_b32"):
        src = args.split(",")
        if len(src) > 1 and src[1].strip() in spills:
            cols.append("reload")
    if op.startswith("s_nop"):
        cols.append("s_nop")
    if op.startswith(_FP64):
        cols.append("fp64")
    return cols


def stamps(lines):
    """[(line index of the s_memtime, slot)] in layout order; slot None where no store with an offset follows the clock read."""
    out = []
    for i, ln in enumerate(lines):
        ins = _instruction(ln)
        if not ins or not ins[0].startswith("s_memtime"):
            continue
        slot = None
        for nx in lines[i + 1:i + 1 + _STAMP_REACH]:
            jn = _instruction(nx)
            if jn and jn[0].startswith("global_store_dwordx2"):
                m = re.search(r"offset:(\d+)", jn[1])
                slot = int(m.group(1)) // 8 if m else 0
                break
        out.append((i, slot))
    return out


def phase_table(asm, prefix):
    """{"spill_vgprs": [...], "phases": [{"from": slot, "to": slot, <column>: count ...}], "loop": {<column>: count}}.
    `loop` is everything between the first and the last stamp."""
    lines = kernel_text(asm, prefix)
    spills = spill_vgprs(lines)
    st = stamps(lines)
    phases = []
    for (a, sa), (b, sb) in zip(st, st[1:]):
        row = {"from": sa, "to": sb}
        row.update({c: 0 for c in COLUMNS})
        for ln in lines[a + 1:b]:
            ins = _instruction(ln)
            if ins:
                for c in classify(ins[0], ins[1], spills):
                    row[c] += 1
        phases.append(row)
    loop = {c: sum(p[c] for p in phases) for c in COLUMNS}
    return {"spill_vgprs": sorted(spills, key=lambda r: int(r[1:]) if r[1:].isdigit() else -1), "phases": phases, "loop": loop}


BLOCK_COLUMNS = COLUMNS + ("lds_read", "div")


def block_table(asm, prefix, slot_from, slot_to):
    """[{"label": ..., <column>: count ...}] for the basic blocks (label to label, layout order) of the first phase that runs from a stamp of
    slot_from to the next stamp, which must be of slot_to; the text in front of the phase's first label counts under "(entry)"."""
    lines = kernel_text(asm, prefix)
    spills = spill_vgprs(lines)
    st = stamps(lines)
    span = next(((a, b) for (a, sa), (b, sb) in zip(st, st[1:]) if sa == slot_from and sb == slot_to), None)
    if span is None:
        raise ValueError("no phase %s->%s" % (slot_from, slot_to))
    rows = [dict({"label": "(entry)"}, **{c: 0 for c in BLOCK_COLUMNS})]
    for ln in lines[span[0] + 1:span[1]]:
        t = ln.split(";")[0].strip()
        if t.endswith(":") and " " not in t:
            rows.append(dict({"label": t[:-1]}, **{c: 0 for c in BLOCK_COLUMNS}))
            continue
        ins = _instruction(ln)
        if not ins:
            continue
        for c in classify(ins[0], ins[1], spills):
            rows[-1][c] += 1
        if ins[0].startswith("ds_read"):
            rows[-1]["lds_read"] += 1
        if ins[0].startswith("v_div_fixup"):
            rows[-1]["div"] += 1
    return rows


def render_blocks(rows):
    out = ["%-14s" % "block" + "".join("%9s" % c for c in BLOCK_COLUMNS)]
    for r in rows:
        out.append("%-14s" % r["label"] + "".join("%9d" % r[c] for c in BLOCK_COLUMNS))
    out.append("%-14s" % "phase" + "".join("%9d" % sum(r[c] for r in rows) for c in BLOCK_COLUMNS))
    return "\n".join(out)


def render(table):
    head = "%-10s" % "stamps" + "".join("%8s" % c for c in COLUMNS)
    rows = [head]
    for p in table["phases"]:
        rows.append("%-10s" % ("%s->%s" % (p["from"], p["to"])) + "".join("%8d" % p[c] for c in COLUMNS))
    rows.append("%-10s" % "first->last" + "".join("%8d" % table["loop"][c] for c in COLUMNS))
    rows.append("spill VGPRs: " + (" ".join(table["spill_vgprs"]) or "none"))
    return "\n".join(rows)


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    if "--blocks" in sys.argv[3:]:
        at = sys.argv.index("--blocks")
        rows = block_table(open(sys.argv[1]).read(), sys.argv[2], int(sys.argv[at + 1]), int(sys.argv[at + 2]))
        print(json.dumps(rows, indent=1) if "--json" in sys.argv[3:] else render_blocks(rows))
        sys.exit(0)
    tab = phase_table(open(sys.argv[1]).read(), sys.argv[2])
    print(json.dumps(tab, indent=1) if "--json" in sys.argv[3:] else render(tab))
