"""Before -> after table of the per-kernel resources of libgatsspg_hip.so from two `-Rpass-analysis=kernel-resource-usage` logs
(`python -m onepose_amd.build_ext --remarks` prints one; cross-compiled for gfx950, no GPU needed).

    python tools/kernel_resources_diff.py BEFORE.txt AFTER.txt > profiles/gats_frames_kernel_resources.txt

A kernel that gained the layout type as a trailing template argument is matched with its former self by dropping that argument:
`k<..., gatsspg::ColLayout>` is the kernel the existing entry points launch, `k<..., gatsspg::FramesLayout>` a new instantiation.
"""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[key] = val
    names = list(out)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    return {re.sub(r"\s+>", ">", re.sub(r"\(.*$", "", d.replace("void ", "", 1))): out[n] for n, d in zip(names, dem)}


def former(name):
    return re.sub(r"<gatsspg::ColLayout>$", "", re.sub(r", gatsspg::ColLayout>$", ">", name))


def main(before, after):
    b, a = parse(before), parse(after)
    a_old = {former(n): (n, r) for n, r in a.items() if "FramesLayout" not in n}
    a_old.update({n: (n, r) for n, r in a.items()})   # a kernel that had its layout argument before is matched by its full name
    print("# kernel | " + " | ".join(FIELDS) + "   (before -> after; '=' unchanged)")
    moved = 0
    for name in sorted(b):
        if name not in a_old:
            print(f"{name} | REMOVED")
            moved += 1
            continue
        cells = []
        for f in FIELDS:
            x, y = b[name].get(f, "?"), a_old[name][1].get(f, "?")
            cells.append(f"{x} =" if x == y else f"{x} -> {y}")
            moved += x != y
        print(f"{name} | " + " | ".join(cells))
    print(f"# existing kernels: {len(b)}; resource figures that moved: {moved}")
    print("# new kernels and instantiations:")
    for name in sorted(a):
        if name not in b and ("FramesLayout" in name or former(name) not in b):
            print(f"{name} | " + " | ".join(a[name].get(f, "?") for f in FIELDS))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
