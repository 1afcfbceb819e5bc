"""Compare the gfx950 instruction streams of every kernel of two builds of the library's objects.

    python profiles/compare_kernel_streams.py OLD/recommend.o NEW/recommend.o
    python profiles/compare_kernel_streams.py OLD_DIR NEW_DIR          # every *.o of OLD_DIR against its namesake

Both objects are taken apart with llvm-objdump (--offloading, then -t and -d on the gfx950 code object).  The kernels
are the symbols that have a kernel descriptor (NAME.kd).  A kernel is keyed by its demangled name (llvm-cxxfilt, or
c++filt); kernels that are left over on both sides - the mangled names differ between the builds when a template or a
function parameter was added - are keyed by name and template arguments with trailing zeros / `false` dropped and the parameter
list left out: a flag that did not exist is a flag that is off.  Two kernels are equal when their instructions AND their
encodings are, line by line (addresses dropped, branch offsets kept).  A kernel only the new build has is counted, one
only the old build has is reported under its object's line.  Prints one line per object and a total; exit status 1
when a kernel that both builds have differs, when an object of the old directory has no namesake in the new one, or
when nothing was compared.  (DESIGN.md sections 19, 26, 27, 28 and 31 record outcomes.)"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
OBJDUMP = os.path.join(LLVM, "llvm-objdump")
# the ROCm toolchain's demangler where it ships one, else the one of binutils: the Itanium names are the same
CXXFILT = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("llvm-cxxfilt") or shutil.which("c++filt")


def loose_key(name):
    """`name<args>(params)` -> `name<args without trailing zeros>`."""
    m = re.match(r"^(?:void )?(.*?)<(.*)>\(.*\)$", name)
    if not m:
        return name.split("(")[0]
    args = m.group(2).split(", ")
    while args and args[-1] in ("0", "false"):
        args.pop()
    return f"{m.group(1)}<{', '.join(args)}>"


def kernels(obj):
    """{demangled kernel name: [(instruction, encoding), ...]} of the gfx950 kernels in `obj`."""
    out = {}
    with tempfile.TemporaryDirectory() as work:
        shutil.copy(obj, os.path.join(work, "in.o"))
        subprocess.run([OBJDUMP, "--offloading", "in.o"], cwd=work, check=True, stdout=subprocess.DEVNULL)
        for f in sorted(os.listdir(work)):
            if "amdgcn" not in f or "gfx950" not in f or os.path.getsize(os.path.join(work, f)) == 0:
                continue
            run = lambda *cmd, **kw: subprocess.run(cmd, cwd=work, check=True, capture_output=True, text=True,  # noqa: E731
                                                    **kw).stdout
            symbols = [line.split()[-1] for line in run(OBJDUMP, "-t", f).splitlines() if line.rstrip().endswith(".kd")]
            mangled = [s[:-3] for s in symbols]
            names = dict(zip(mangled, run(CXXFILT, input="\n".join(mangled)).splitlines()))
            cur = None
            for line in run(OBJDUMP, "-d", f).splitlines():
                if not line.startswith("\t"):
                    m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line.strip())
                    cur = None
                    if m and m.group(1) in names:
                        cur = out[names[m.group(1)]] = []
                    continue
                if cur is not None and "//" in line:
                    ins, enc = line.split("//", 1)
                    # a branch's annotation names its target as <kernel symbol+offset>: keep the offset
                    enc = re.sub(r"<\S+?(\+0x[0-9a-f]+)?>", r"<\1>", enc.split(":", 1)[1].strip())
                    cur.append((ins.strip(), enc))
    return out


def compare(old, new, label):
    """Prints the line of one pair of objects; returns (identical, differing, missing, new, instructions)."""
    a, b = kernels(old), kernels(new)
    pairs = [(k, k) for k in a if k in b]
    # the leftovers by loose key; a loose key that two kernels of one side share pairs nothing
    left_a, left_b = {}, {}
    for side, other, left in ((a, b, left_a), (b, a, left_b)):
        for k in side:
            if k not in other:
                left.setdefault(loose_key(k), []).append(k)
    loose = [k for k in left_a if k in left_b and len(left_a[k]) == 1 and len(left_b[k]) == 1]
    pairs += [(left_a[k][0], left_b[k][0]) for k in loose]
    missing = sorted(n for k, names in left_a.items() if k not in loose for n in names)
    fresh = sorted(n for k, names in left_b.items() if k not in loose for n in names)
    differing = [(ka, kb) for ka, kb in sorted(pairs) if a[ka] != b[kb]]
    ninstr = sum(len(a[ka]) for ka, _ in pairs)
    print(f"{label}: {len(a)} kernels in the old build, {len(b)} in the new ({len(fresh)} new, {len(missing)} missing); "
          f"{len(pairs) - len(differing)} identical, {len(differing)} not; {ninstr} instructions compared")
    for ka, kb in differing:
        print(f"  {label}: differs: {ka}: {len(a[ka])} -> {len(b[kb])} instructions")
    for k in missing:
        print(f"  {label}: missing in the new build: {k}")
    return len(pairs) - len(differing), len(differing), len(missing), len(fresh), ninstr


def main(old, new):
    if os.path.isdir(old):
        files = sorted(f for f in os.listdir(old) if f.endswith(".o"))
        absent = [f for f in files if not os.path.exists(os.path.join(new, f))]
        for f in absent:
            print(f"{f}: not in the new build")
        jobs = [(os.path.join(old, f), os.path.join(new, f), f) for f in files if os.path.exists(os.path.join(new, f))]
    else:
        absent, jobs = [], [(old, new, os.path.basename(new))]
    tot = [0] * 5
    for job in jobs:
        tot = [t + r for t, r in zip(tot, compare(*job))]
    if len(jobs) > 1:
        print(f"total: {len(jobs)} objects, {len(absent)} not in the new build; {tot[0]} kernels identical, {tot[1]} not, "
              f"{tot[2]} missing in the new build, {tot[3]} new; {tot[4]} instructions compared")
    return 1 if tot[1] or absent or not tot[0] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
