"""Device-ISA comparison of two TREES (e.g. an export of the parent commit and this one), kernel by kernel, on the CPU.

    python scripts/ubench/isa_identity.py TREE_A TREE_B [file.hip ...]     # default: pe.hip geom.hip pointnet2.hip posehead.hip

Every file is compiled with the product flags (`build.FLAGS + EXTRA_FLAGS[file]`, `-S --cuda-device-only`); lines that carry the
per-file `__hip_cuid_` symbol are dropped.  A file is "identical" as a whole, or its kernels are compared one by one between the
`_Z...:` label and `.Lfunc_end`; for a kernel that differs the `-Rpass-analysis=kernel-resource-usage` lines of both sides follow.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unopose_amd import build  # noqa: E402


def compile_isa(tree, f):
    r = subprocess.run([build._hipcc(), *build.FLAGS, *build.EXTRA_FLAGS.get(f, []), "-Rpass-analysis=kernel-resource-usage", "-S",
                        "--cuda-device-only", os.path.join(tree, "unopose_amd", "csrc", f), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if "__hip_cuid_" not in l]
    kernels, name = {}, None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m and name is None:
            name = m.group(1)
            kernels[name] = []
        if name is not None:
            kernels[name].append(l)
            if l.startswith(".Lfunc_end"):
                name = None
    usage, name = {}, None
    for l in r.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+((?:VGPRs|ScratchSize|Occupancy) ?(?:\[[^\]]*\])?:\s*\d+))", l)
        if m and m.group(1):
            name = m.group(1)
        elif m and name:
            usage.setdefault(name, []).append(" ".join(m.group(2).split()))
    return lines, kernels, usage


def main():
    a, b = sys.argv[1:3]
    files = sys.argv[3:] or ["pe.hip", "geom.hip", "pointnet2.hip", "posehead.hip"]
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(lambda j: compile_isa(*j), [(t, f) for f in files for t in (a, b)]))
    for i, f in enumerate(files):
        (la, ka, ua), (lb, kb, ub) = res[2 * i], res[2 * i + 1]
        print(f"{f}: {'identical as a whole' if la == lb else 'differs'} ({len(la)} / {len(lb)} lines of ISA)")
        if la == lb:
            continue
        for k in sorted(set(ka) | set(kb)):
            pretty = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip().split("(")[0]
            if ka.get(k) == kb.get(k):
                print(f"    {pretty}: identical")
            else:
                print(f"    {pretty}: DIFFERS  ({len(ka.get(k, []))} / {len(kb.get(k, []))} lines)\n"
                      f"        A: {'; '.join(ua.get(k, []))}\n        B: {'; '.join(ub.get(k, []))}")


if __name__ == "__main__":
    main()
