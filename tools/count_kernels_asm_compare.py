"""Developer tool: the gfx950 device code of the count kernels of two source trees, same-named kernel by kernel (no GPU: hipcc
cross-compiles).  For a change that is meant to leave the kernels as they are: a refactor of the software pipeline, of the
headers they share.  The logs it has printed are profiles/*_asm_compare.log.

Every translation unit that includes scan_tiles.h in THIS tree is compiled to assembly in both trees with the Makefile's flags.
Label numbers are normalised.  A kernel that comes out identical (instructions and statistics) says so.  One that does not must
be a software-pipelined kernel (non-temporal loads, a counted vmcnt(N) wait, two vmcnt(0) waits that land both register sets), and is compared
structurally: VGPRs, AGPRs, LDS and occupancy equal, no scratch, no VGPR spills, the same s_waitcnt vmcnt(N) census, no more
vmcnt(0) waits inside the pipeline (first non-temporal load .. that pair of waits) than the parent, and the same number of
global_load, ds_* and v_cmp* instructions in it.  SGPRs, SGPR spills to VGPR lanes (v_writelane / v_readlane, no memory) and
the other opcodes may differ: they are printed, with the register-masked diff.  Any other kernel that differs fails.  Kernels that only one tree has are listed.
usage: count_kernels_asm_compare.py PARENT_TREE [THIS_TREE]"""
import collections, difflib, os, re, subprocess, sys

PKG = "adhoc-queries-pointclouds_amd"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Wno-unused-parameter",
         "-S", "--cuda-device-only"]  # csrc/Makefile CXXFLAGS (its -I. is the csrc directory given below)
EQUAL = ("NumVgprs", "NumAgprs", "LDSByteSize", "Occupancy")
ZERO = ("ScratchSize", "vgpr_spill_count")
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


def vmcnt(l):
    m = re.search(r"s_waitcnt.*vmcnt\((\d+)\)", l)
    return int(m.group(1)) if m else None


def pipeline(body):
    """first non-temporal load .. the second vmcnt(0) wait behind the last counted wait of the loop (the deepest vmcnt(N) of the
    kernel): pipe_wait<0> of A and of B.  Empty for a kernel without them."""
    nt = [i for i, l in enumerate(body) if l.startswith("global_load") and l.endswith(" nt")]
    depth = max([vmcnt(l) or 0 for l in body] or [0])
    if not nt or not depth:
        return []
    last = max(i for i, l in enumerate(body) if vmcnt(l) == depth)
    zeros = [i for i in range(last, len(body)) if vmcnt(body[i]) == 0]
    return body[nt[0]:zeros[1] + 1] if len(zeros) >= 2 else []


def family(hist):
    """the opcodes that must not change in number: loads, LDS operations, compares"""
    out = collections.Counter()
    for op, n in hist.items():
        for f in ("global_load", "ds_", "v_cmp"):
            if op.startswith(f):
                out[f + "*"] += n
    return dict(sorted(out.items()))


def main():
    parent, this = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.isdir(os.path.join(parent, PKG, "csrc")), "no source tree at " + parent
    old, new = {}, {}
    for u in units(this):
        new.update({(u, k): v for k, v in kernels(this, u).items()})
        if os.path.exists(os.path.join(parent, PKG, "csrc", u)):
            old.update({(u, k): v for k, v in kernels(parent, u).items()})
    print("units:", " ".join(units(this)))
    ok = True
    for key in sorted(set(old) - set(new)):
        print("only in parent:   %s :: %s" % key)
    for key in sorted(set(new) - set(old)):
        print("only in this tree: %s :: %s" % key)
    for (u, name) in sorted(set(old) & set(new)):
        (body, st), (nbody, nst) = old[(u, name)], new[(u, name)]
        if normal(body) == normal(nbody) and st == nst:
            print("identical %s :: %s  (%d instructions)" % (u, name, len([l for l in body if opcode(l)])))
            continue
        pa, pb = pipeline(body), pipeline(nbody)
        if not pa or not pb:
            print("DIFFERS   %s :: %s  (no software pipeline: it must be identical)" % (u, name))
            ok = False
            continue
        print("\n== %s :: %s" % (u, name))
        good = all(st.get(k) == nst.get(k) for k in EQUAL) and all(nst.get(k, 0) == 0 for k in ZERO)
        print("   statistics      parent %s\n                   this   %s   %s" % (st, nst, "as required" if good else "NOT as required"))
        print("   vmcnt census    parent %s\n                   this   %s   %s" % (waits(body), waits(nbody), "same" if waits(body) == waits(nbody) else "DIFFER"))
        good &= waits(body) == waits(nbody)
        ha, hb = (collections.Counter(filter(None, map(opcode, p))) for p in (pa, pb))
        inside = lambda p: sum(1 for l in p if vmcnt(l) == 0) - 2
        print("   pipeline        parent %d instructions, this %d; vmcnt(0) inside: parent %d, this %d" % (sum(ha.values()), sum(hb.values()), inside(pa), inside(pb)))
        print("                   loads, LDS, compares: parent %s, this %s   %s" % (family(ha), family(hb), "same" if family(ha) == family(hb) else "DIFFER"))
        print("                   other opcodes: parent only %s, this only %s" % (dict(ha - hb), dict(hb - ha)))
        good &= family(ha) == family(hb) and inside(pb) <= inside(pa)
        whole = (collections.Counter(filter(None, map(opcode, body))), collections.Counter(filter(None, map(opcode, nbody))))
        print("   whole kernel    parent %d instructions, this %d; parent only %s, this only %s" %
              (sum(whole[0].values()), sum(whole[1].values()), dict(whole[0] - whole[1]), dict(whole[1] - whole[0])))
        d = [l for l in difflib.unified_diff(normal(body, True), normal(nbody, True), "parent", "this", n=2, lineterm="")]
        print("   with registers masked: %s" % ("identical" if not d else "%d diff lines" % len(d)))
        for l in d[:120]:
            print("      " + l)
        print("   -> %s" % ("as required" if good else "NOT AS REQUIRED"))
        ok &= good
    print("\nRESULT:", "as required" if ok else "DIFFERENCES, see above")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
