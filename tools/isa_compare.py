"""Are the gfx950 kernels of two builds of csrc/ the same machine code?  For a change that only moves kernels between source files.
usage: python tools/isa_compare.py PARENT_CSRC HEAD_CSRC [objects whose kernels are listed one by one, or `all`; default dffw_srd_roll.o]

Both directories hold a finished `make` (objects + ../libdffw.so).  Per kernel of the parent's object: the kernel of the same name in
the head's objects, its instruction stream (llvm-objdump -d without addresses, encodings and symbol offsets) and its resource notes
(registers, LDS, scratch, spills) compared -> `same` / `differs`.  Then the kernel symbol sets of the two libraries and the sha256 of
every object.  Exit status 1 when a kernel differs or is missing or the symbol sets differ."""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin/"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
NOTES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def code_objects(path, tmp):
    """the gfx950 code objects inside the .hip_fatbin section of an object or library (a library holds one bundle per translation unit)"""
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([LLVM + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat], check=True)
    blob = open(fat, "rb").read() if os.path.exists(fat) else b""
    starts = [m.start() for m in re.finditer(MAGIC, blob)]
    out = []
    for i, s in enumerate(starts):
        one, co = os.path.join(tmp, "one.bin"), os.path.join(tmp, "%s.%d.co" % (os.path.basename(path), i))
        open(one, "wb").write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.run([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + one, "--output=" + co], check=True)
        if os.path.getsize(co):
            out.append(co)
    return out


def kernel_notes(co):
    """{mangled kernel name: {note: value}} of one code object (the entries of its metadata that carry an argument list: an argument's own
    `.name:` is not a kernel)"""
    notes = {}
    for block in re.split(r"\n  - (?=\.)", run(LLVM + "llvm-readelf", "--notes", co)):
        name = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
        if name and ".args:" in block:
            notes[name.group(1)] = {k: (re.search(r"^\s*%s:\s+(\S+)" % re.escape(k), block, re.M) or [0, "0"])[1] for k in NOTES}
    return notes


def kernels(path, tmp):
    """{mangled kernel name: (instruction lines, {note: value})} of one object or library"""
    res = {}
    for co in code_objects(path, tmp):
        notes = kernel_notes(co)
        cur = None
        for line in run(LLVM + "llvm-objdump", "-d", co).splitlines():
            m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = res.setdefault(m.group(1), ([], notes.get(m.group(1)))) if m.group(1) in notes else None
            elif cur is not None and line.startswith("\t") and line.strip() != "...":   # ("...": zero padding up to the next symbol's alignment)
                cur[0].append(re.sub(r"\s*<[^>]*>\s*$", "", line.split("//")[0].strip()))
    return res


def main():
    parent, head = sys.argv[1], sys.argv[2]
    listed = sys.argv[3:] or ["dffw_srd_roll.o"]
    if listed == ["all"]:
        listed = sorted(os.path.basename(o) for o in glob.glob(os.path.join(parent, "*.o")))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old = {}
        for o in listed:
            old.update(kernels(os.path.join(parent, o), tmp))
        new = {}
        for o in sorted(glob.glob(os.path.join(head, "*.o"))):
            for k, v in kernels(o, tmp).items():
                new[k] = v + (os.path.basename(o),)
        print("kernels of the parent's %s against the kernel of the same name in the head's objects (gfx950)" % " ".join(listed))
        print("%-62s %6s %4s %4s %4s %6s %7s %6s  %-16s %s" % ("kernel", "insns", "VGPR", "AGPR", "SGPR", "LDS", "scratch", "spills", "head object", ""))
        names = {k: run("c++filt", k).strip() for k in old}
        for k in sorted(old, key=names.get):
            ins, nt = old[k]
            name = re.sub(r"\(.*", "", names[k]).replace("void dffw::", "")
            h = new.get(k)
            same = h is not None and h[0] == ins and h[1] == nt
            bad += not same
            print("%-62s %6d %4s %4s %4s %6s %7s %6s  %-16s %s" % (name, len(ins), nt[NOTES[0]], nt[NOTES[1]], nt[NOTES[2]], nt[NOTES[3]], nt[NOTES[4]],
                                                              nt[NOTES[5]] + "/" + nt[NOTES[6]], h[2] if h else "-", "same" if same else "differs" if h else "MISSING"))
        print("%d kernels listed, %d not the same" % (len(old), bad))
        lib_old, lib_new = (set(kernels(os.path.join(d, "..", "libdffw.so"), tmp)) for d in (parent, head))
        print("\nkernel symbols in libdffw.so: parent %d, head %d, only in parent %s, only in head %s" % (len(lib_old), len(lib_new), sorted(lib_old - lib_new), sorted(lib_new - lib_old)))
        bad += lib_old != lib_new
    sha = lambda d: {os.path.basename(o): hashlib.sha256(open(o, "rb").read()).hexdigest() for o in glob.glob(os.path.join(d, "*.o"))}
    a, b = sha(parent), sha(head)
    print("\nsha256 of the objects (parent, head)")
    for o in sorted(set(a) | set(b)):
        print("%-64s %-64s %-22s %s" % (a.get(o, "-"), b.get(o, "-"), o, "same" if a.get(o) == b.get(o) else "new" if o not in a else "differs"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
