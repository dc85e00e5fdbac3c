"""Developer tool: the gfx950 device code of the count kernels of two source trees, kernel by kernel (no GPU: hipcc
cross-compiles).  Written for the change that made the three batched K1 kernels one template (scan_tiles.h); the log it
prints is profiles/batch_k1_asm_compare.log.

Every translation unit that includes scan_tiles.h is compiled to assembly in both trees with the Makefile's flags.  Symbol
names and label numbers are normalised.  A kernel that is the same source in both trees must come out identical.  For the
batched K1 instantiations (and the finish reduction, which had four names) the register allocator may rename, so they are
compared structurally: registers, scratch, spills, occupancy, the s_waitcnt vmcnt(N) census, and the opcode histogram of the
software pipeline (first non-temporal load .. the pair of vmcnt(0) waits that lands both register sets); what still differs is
printed with registers masked.
Tied to that one pair of commits: RENAMED and UNITS below name the kernels and files that change replaced, so PARENT_TREE is
a checkout of the commit before it; another comparison needs another mapping.
usage: batch_k1_asm_compare.py PARENT_TREE [THIS_TREE]"""
import collections, difflib, os, re, subprocess, sys

PKG = "adhoc-queries-pointclouds_amd"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Wno-unused-parameter",
         "-S", "--cuda-device-only"]  # csrc/Makefile CXXFLAGS (its -I. is the csrc directory given below)
BATCH = "k_bounds_count_batch_pipe"
# parent kernel (a part of its mangled name) -> this tree's
RENAMED = {"31k_bounds_class_count_batch_pipeILi2EE": "25k_bounds_count_batch_pipeILi2EJNS_10ClassBytesEEE",
           "30k_bounds_time_count_batch_pipeILi2EE": "25k_bounds_count_batch_pipeILi2EJNS_8GpsTimesEEE",
           "25k_bounds_count_batch_pipeILi2EE": "25k_bounds_count_batch_pipeILi2EJEE",
           "23k_finish_count_combinedE": "14k_finish_countE", "26k_finish_count_bounds_timeE": "14k_finish_countE",
           "14k_index_finishE": "14k_finish_countE"}
UNITS = {"scan_count_combined.hip": "scan_count_batch.hip", "scan_count_bounds_time.hip": "scan_count_batch.hip"}
STATS = ("NumSgprs", "TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "sgpr_spill_count", "vgpr_spill_count", "LDSByteSize")


def units(tree):
    d = os.path.join(tree, PKG, "csrc")
    return sorted(f for f in os.listdir(d) if f.endswith(".hip") and "scan_tiles.h" in open(os.path.join(d, f)).read())


def kernels(tree, unit):
    """mangled name -> (instruction lines without comments, statistics)"""
    out = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, PKG, "csrc"), "-o", "-",
                          os.path.join(tree, PKG, "csrc", unit)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    spills, cur = {}, None  # the kernels' metadata: .name, .sgpr_spill_count, .vgpr_spill_count in that order
    for l in lines:
        m = re.match(r"^\s+\.(name|sgpr_spill_count|vgpr_spill_count):\s+(\S+)", l)
        if m and m.group(1) == "name":
            cur = m.group(2)
        elif m:
            spills.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    found, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m:
            i += 1
            continue
        j = i + 1
        while not lines[j].startswith(".Lfunc_end"):
            j += 1
        body = [l.split(";")[0].strip() for l in lines[i + 1:j]]
        body = [l for l in body if l and not l.startswith(".") or l.startswith(".LBB") and l.endswith(":")]
        st = {}
        for l in lines[j:j + 40]:
            s = re.match(r"^; (\w+): (\d+)", l)
            if s and s.group(1) in STATS:
                st[s.group(1)] = int(s.group(2))
        st.update(spills.get(m.group(1), {}))
        found[m.group(1)] = (body, st)
        i = j
    return found


def normal(body, mask=False):
    labels, out = {}, []
    for l in body:
        l = re.sub(r"_Z\w+", "SYM", l)
        l = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), l)
        if mask:
            l = re.sub(r"\b([vsa])\[(\d+):(\d+)\]", lambda m: "%s[%d]" % (m.group(1), int(m.group(3)) - int(m.group(2)) + 1), l)
            l = re.sub(r"\b([vsa])\d+\b", r"\1#", l)
        out.append(l)
    return out


def opcode(l):
    return l.split()[0] if not l.endswith(":") else None


def waits(body):
    return dict(sorted(collections.Counter(m.group(1) for l in body for m in [re.search(r"s_waitcnt.*(vmcnt\(\d+\))", l)] if m).items()))


def pipeline(body):
    """first non-temporal load .. the second of the two adjacent vmcnt(0) waits behind the last one (pipe_wait<0> of A and of B)"""
    nt = [i for i, l in enumerate(body) if l.startswith("global_load") and l.endswith(" nt")]
    if not nt:
        return []
    end = next(i for i in range(nt[-1], len(body) - 1) if body[i] == body[i + 1] == "s_waitcnt vmcnt(0)") + 1
    return body[nt[0]:end + 1]


def main():
    parent, this = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    old, new = {}, {}
    for u in units(parent):
        old.update({(u, k): v for k, v in kernels(parent, u).items()})
    for u in units(this):
        new.update({(u, k): v for k, v in kernels(this, u).items()})
    print("parent units:", " ".join(units(parent)))
    print("this tree's: ", " ".join(units(this)))
    ok = True
    for (u, name), (body, st) in sorted(old.items()):
        to = name
        for a, b in RENAMED.items():
            to = to.replace(a, b)
        cand = [k for k in new if k == (UNITS.get(u, u), to)]
        if len(cand) != 1:
            print("MISSING in this tree:", u, name)
            ok = False
            continue
        nbody, nst = new[cand[0]]
        if to == name:
            same = normal(body) == normal(nbody) and st == nst
            print("%-9s %s :: %s  (%d instructions)" % ("identical" if same else "DIFFERS", u, name, len([l for l in body if opcode(l)])))
            ok &= same
            continue
        print("\n== %s :: %s\n-> %s :: %s" % (u, name, cand[0][0], to))
        print("   statistics      parent %s\n                   this   %s   %s" % (st, nst, "same" if st == nst else "DIFFER"))
        print("   vmcnt census    parent %s\n                   this   %s   %s" % (waits(body), waits(nbody), "same" if waits(body) == waits(nbody) else "DIFFER"))
        ni, nn = len([l for l in body if opcode(l)]), len([l for l in nbody if opcode(l)])
        print("   instructions    parent %d, this %d" % (ni, nn))
        ok &= st == nst and waits(body) == waits(nbody)
        if BATCH[2:] in to:
            pa, pb = pipeline(body), pipeline(nbody)
            ha, hb = (collections.Counter(filter(None, map(opcode, p))) for p in (pa, pb))
            inside = lambda p: sum(1 for l in p[:-2] if "vmcnt(0)" in l)
            print("   pipeline        parent %d instructions, this %d; opcode histogram %s; vmcnt(0) inside: parent %d, this %d" %
                  (sum(ha.values()), sum(hb.values()), "same" if ha == hb else "DIFFERS %s" % ((ha - hb) + (hb - ha)), inside(pa), inside(pb)))
            ok &= ha == hb and inside(pb) <= inside(pa)
        whole = (collections.Counter(filter(None, map(opcode, body))), collections.Counter(filter(None, map(opcode, nbody))))
        print("   whole kernel    opcode histogram %s" % ("same" if whole[0] == whole[1] else "differs: parent only %s, this only %s" %
                                                          (dict(whole[0] - whole[1]), dict(whole[1] - whole[0]))))
        differ = sum(a != b for a, b in zip(normal(body), normal(nbody))) if len(body) == len(nbody) else None
        print("   with registers as allocated: %s" % ("identical" if differ == 0 else "%s of %d lines differ" % (differ, len(body))))
        d = [l for l in difflib.unified_diff(normal(body, True), normal(nbody, True), "parent", "this", n=2, lineterm="")]
        print("   with registers masked: %s" % ("identical" if not d else "%d diff lines" % len(d)))
        for l in d[:200]:
            print("      " + l)
    for k in sorted(new):
        if not any(k[1] == n or any(b in k[1] for b in RENAMED.values()) for (_, n) in old):
            print("NEW in this tree:", k)
    print("\nRESULT:", "as required" if ok else "DIFFERENCES, see above")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
