"""Per-kernel comparison of two gfx950 assembly files (hipcc --save-temps / -S) and, for kernels that differ, their resource remarks."""
import re, sys
def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body; name = None
            else:
                body.append(re.sub(r"\s*;.*$", "", line.rstrip()))
    return out
def resources(path):
    out = {}
    for block in re.split(r"Function Name: ", open(path).read())[1:]:
        name = block.split()[0]
        get = lambda what: int(re.search(what + r": (\d+)", block).group(1))
        out[name] = dict(vgpr=get(r" VGPRs"), agpr=get(r"AGPRs"), sgpr=get(r"TotalSGPRs"), occ=get(r"Occupancy \[waves/SIMD\]"), scratch=get(r"ScratchSize \[bytes/lane\]"), lds=get(r"LDS Size \[bytes/block\]"))
    return out
def count(body, pat): return sum(1 for l in body if re.search(pat, l))
def commuted(body):
    """The body with the two sources of every v_add_f64 / v_mul_f64 in sorted order: IEEE addition and multiplication commute."""
    out = []
    for l in body:
        m = re.match(r"^(\s*v_(?:add|mul)_f64 \S+, )(\S+), (\S+)$", l)
        out.append(m.group(1) + ", ".join(sorted(m.group(2, 3))) if m else l)
    return out
pa, ta, pr, tr = sys.argv[1:5]
P, T, PR, TR = kernels(pa), kernels(ta), resources(pr), resources(tr)
print("kernels: parent %d, this tree %d; names only in one: %s" % (len(P), len(T), sorted(set(P) ^ set(T))))
same = [k for k in P if k in T and P[k] == T[k]]
diff = [k for k in P if k in T and P[k] != T[k]]
print("identical line for line (comments stripped): %d" % len(same))
for k in sorted(same):
    if "fold_kernel" in k: print("  identical  %s" % k)
print("different: %d" % len(diff))
for k in sorted(diff):
    print("  DIFFERENT  %s%s" % (k, "   (only in the order of the two sources of v_add_f64 / v_mul_f64)" if commuted(P[k]) == commuted(T[k]) else ""))
    for tag, A, R in (("parent", P, PR), ("tree  ", T, TR)):
        b = A[k]
        print("      %s lines %5d  s_load %3d  s_buffer_load %d  global_load %3d  global_store %3d  v_div/rcp/fma_f64 %d  %s" % (
            tag, len(b), count(b, r"^\s*s_load_"), count(b, r"^\s*s_buffer_load"), count(b, r"^\s*global_load"), count(b, r"^\s*global_store"),
            count(b, r"^\s*v_(div|rcp|fma)\w*_f64"), R.get(k)))
