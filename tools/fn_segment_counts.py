"""Static instruction counts of k_find_neighbors per stamped segment. Compile csrc/sph_neighbors.hip with the Makefile's HIPFLAGS
plus `-DFN_STAMPS --cuda-device-only -S` and pass the .s file(s): each instance is split at its s_memtime reads (every FN_STAMP
reads the clock twice; the instructions between the second read of one stamp and the first read of the next are that segment's)
and VALU, packed, LDS, global and s_nop instructions are counted per segment. Static counts in program order: code that the
compiler moved across a stamp is counted where it landed, loops count once. The labels follow the order of the clock reads in
the file: where hipcc lays the blocks of an instance out of source order (k_find_neighbors<true>) the segments shift against the
labels and are told apart by their content (the bisection is the one of about 140 VALU in a loop of five trips)."""
import re
import sys

SEG = ["head", "loads+barrier", "setup", "walk", "expand", "bisect", "pass1+store", "exact walks", "rest"]


def kernels(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z16k_find_neighborsILb([01])E\w*):", line)
        if m:
            name, body = "<true>" if m.group(2) == "1" else "<false>", []
            continue
        if name and line.startswith(".Lfunc_end"):
            yield name, body
            name = None
        elif name:
            body.append(line.strip())


def count(body):
    segs, cur, reads = [], dict(valu=0, pk=0, lds=0, glob=0, nop=0), 0
    for ins in body:
        op = ins.split()[0] if ins else ""
        if op.startswith("s_memtime"):
            reads += 1
            if reads == 1 or reads % 2 == 0:  # read 1 ends the prologue; the first read of a stamp closes its segment
                segs.append(cur)
            cur = dict(valu=0, pk=0, lds=0, glob=0, nop=0)  # (the second read opens the next: the stamp's own atomic is dropped)
            continue
        if op.startswith("v_"):
            cur["valu"] += 1
            cur["pk"] += op.startswith("v_pk_")
        elif op.startswith("ds_"):
            cur["lds"] += 1
        elif op.startswith("global_") or op.startswith("buffer_") or op.startswith("flat_"):
            cur["glob"] += 1
        elif op == "s_nop":
            cur["nop"] += 1
    segs.append(cur)
    return segs


for path in sys.argv[1:]:
    for name, body in kernels(path):
        print("%s %s" % (path, name))
        segs = count(body)
        for i, s in enumerate(segs + [{k: sum(t[k] for t in segs) for k in segs[0]}]):
            label = SEG[i - 1] if 1 <= i <= len(SEG) else ("prologue" if i == 0 else "-")
            if i == len(segs):
                label = "whole kernel"
            print("  %-14s VALU %5d (packed %4d)  LDS %4d  global %4d  s_nop %4d" % (label, s["valu"], s["pk"], s["lds"], s["glob"], s["nop"]))
