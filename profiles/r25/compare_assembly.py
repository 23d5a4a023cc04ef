"""Per-kernel comparison of two gfx950 assembly files of wayverb_amd/csrc/engine.hip (hipcc --save-temps) and their resource remarks
(-Rpass-analysis=kernel-resource-usage): parent commit against this tree.  After profiles/r18/compare_assembly.py; what is new is the
verdict this round's issue asks for -- every kernel that does not inline boundary_body identical line for line, and every instantiation
of boundary_kernel / plane_step_kernel / whole_step_kernel either identical or: no register, scratch or LDS figure higher, occupancy
none lower, the same number of global_load* and global_store* instructions.  Exit status 1 if a kernel fails that.
Local labels are compared without the function's index in the module (.LBB185_31 as .LBB_31): the host's table of boundary kernels
instantiates them in another order than the branch chain did, so the compiler emits them in another order and numbers them anew.

usage: compare_assembly.py parent.s tree.s parent_remarks.txt tree_remarks.txt"""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            else:
                body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", re.sub(r"\s*;.*$", "", line.rstrip())))
    return out


def resources(path):
    out = {}
    for block in re.split(r"Function Name: ", open(path).read())[1:]:
        name = block.split()[0]
        get = lambda what: int(re.search(what + r": (\d+)", block).group(1))
        out[name] = dict(vgpr=get(r" VGPRs"), agpr=get(r"AGPRs"), sgpr=get(r"TotalSGPRs"), occ=get(r"Occupancy \[waves/SIMD\]"),
                         scratch=get(r"ScratchSize \[bytes/lane\]"), lds=get(r"LDS Size \[bytes/block\]"))
    return out


def count(body, pat):
    return sum(1 for l in body if re.search(pat, l))


def multiset(body):
    """The instructions of a body with register numbers blanked, sorted: equal for two bodies that differ only in the order of their
    instructions and in which registers the allocator chose."""
    return sorted(re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", l) for l in body if l.strip() and not l.strip().startswith("."))


INLINES_BOUNDARY_BODY = ("boundary_kernel", "plane_step_kernel", "whole_step_kernel")
pa, ta, pr, tr = sys.argv[1:5]
P, T, PR, TR = kernels(pa), kernels(ta), resources(pr), resources(tr)
print("kernels: parent %d, this tree %d; names only in one: %s" % (len(P), len(T), sorted(set(P) ^ set(T))))
same = [k for k in P if k in T and P[k] == T[k]]
diff = [k for k in P if k in T and P[k] != T[k]]
print("identical line for line (comments stripped): %d" % len(same))
for k in sorted(same):
    if any(n in k for n in INLINES_BOUNDARY_BODY):
        print("  identical  %s" % k)
print("different: %d" % len(diff))
failed = bool(set(P) ^ set(T))
for k in sorted(diff):
    print("  DIFFERENT  %s" % k)
    figures = {}
    for tag, A, R in (("parent", P, PR), ("tree  ", T, TR)):
        b = A[k]
        figures[tag] = (count(b, r"^\s*global_load"), count(b, r"^\s*global_store"), R[k])
        print("      %s lines %5d  s_load %3d  global_load %3d  global_store %3d  v_div/rcp/fma_f64 %d  %s" % (
            tag, len(b), count(b, r"^\s*s_load_"), figures[tag][0], figures[tag][1], count(b, r"^\s*v_(div|rcp|fma)\w*_f64"), R[k]))
    (pl, ps, p), (tl, ts, t) = figures["parent"], figures["tree  "]
    ok = (any(n in k for n in INLINES_BOUNDARY_BODY) and all(t[f] <= p[f] for f in ("vgpr", "agpr", "sgpr", "scratch", "lds"))
          and t["occ"] >= p["occ"] and (tl, ts) == (pl, ps))
    print("      same instructions up to their order and the registers chosen: %s" % ("yes" if multiset(P[k]) == multiset(T[k]) else "no"))
    print("      %s" % ("meets the three conditions (no register / scratch / LDS figure higher, occupancy not lower, as many global loads and stores)"
                        if ok else "FAILS"))
    failed = failed or not ok
print("verdict: %s" % ("FAILED" if failed else "every kernel outside boundary_body's three identical; the rest identical or within the conditions"))
sys.exit(1 if failed else 0)
