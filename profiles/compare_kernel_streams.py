"""Compare the gfx950 instruction streams of the k_recommend / k_rank_count instantiations of two builds of
recommend.hip or rank_eval.hip.

    python profiles/compare_kernel_streams.py OLD/recommend.o NEW/recommend.o
    python profiles/compare_kernel_streams.py OLD/rank_eval.o NEW/rank_eval.o

Both objects are taken apart with llvm-objdump (--offloading, then -d on the gfx950 code object).  A kernel is keyed
by its name and template arguments (k_recommend: KB, NW, CAP, MASKED, DEEP, SEG; k_rank_count: KB, NW, MASKED, SEG)
with trailing zeros dropped - the mangled names differ between the builds when a template or a function parameter
was added, and a flag that did not exist is a flag that is off -, and two kernels are equal when their instructions
AND their encodings are, line by line (addresses dropped).  Keys only the new build has are new and only counted.
Exit status 1 when a kernel that both builds have differs.  (DESIGN.md sections 26 and 27 record the outcomes for
als_recommend_deep and als_recommend_topk_segmented.)"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
NAME = re.compile(r"(k_recommend|k_rank_count)I((?:L[ib]\d+E)+)E")


def kernels(obj):
    """{(name, template arguments without trailing zeros): [(instruction, encoding), ...]} of the kernels in `obj`."""
    out, cur = {}, None
    with tempfile.TemporaryDirectory() as work:
        shutil.copy(obj, os.path.join(work, "in.o"))
        subprocess.run([OBJDUMP, "--offloading", "in.o"], cwd=work, check=True, stdout=subprocess.DEVNULL)
        for f in sorted(os.listdir(work)):
            if "amdgcn" not in f or "gfx950" not in f or os.path.getsize(os.path.join(work, f)) == 0:
                continue
            text = subprocess.run([OBJDUMP, "-d", f], cwd=work, check=True, capture_output=True, text=True).stdout
            for line in text.splitlines():
                if not line.startswith("\t"):
                    m = NAME.search(line)
                    cur = None
                    if m and line.rstrip().endswith(">:"):
                        args = [int(g) for g in re.findall(r"L[ib](\d+)E", m.group(2))]
                        while args and args[-1] == 0:
                            args.pop()
                        cur = (m.group(1), *args)
                        out[cur] = []
                    continue
                if cur is not None and "//" in line:
                    ins, enc = line.split("//", 1)
                    # a branch's annotation names its target as <kernel symbol+offset>: keep the offset
                    enc = re.sub(r"<\S+?(\+0x[0-9a-f]+)?>", r"<\1>", enc.split(":", 1)[1].strip())
                    out[cur].append((ins.strip(), enc))
    return out


def main(old, new):
    a, b = kernels(old), kernels(new)
    fresh = [k for k in b if k not in a]
    same = differ = 0
    for key in sorted(a):
        if key not in b:
            print("missing in the new build:", key)
            differ += 1
        elif a[key] != b[key]:
            print("differs:", key, len(a[key]), "->", len(b[key]), "instructions")
            differ += 1
        else:
            same += 1
    print(f"{len(a)} kernels in the old build, {len(b)} in the new ({len(fresh)} new); {same} identical, "
          f"{differ} not; {sum(len(v) for v in a.values())} instructions compared")
    return 1 if differ or not a else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
