#!/usr/bin/env python
"""Kernel time of the DAC baseline's adversarial step by family, from the kernel_stats.csv of one counter-free kernel trace

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o adv -- python tools/dac_adv_timing.py --steps 4 --only dac_tiny --arm adv
    python tools/dac_adv_kernels.py DIR/.../adv_kernel_stats.csv 4 "DAC-Tiny 16 x 3 s" [more csv/steps/title triples] > profiles/dac_adv_kernels.txt

libescx's kernels (namespace escx) are one line; every other family - what the composition itself adds around them - is listed with its share of the step's
kernel time: torch.cat of [fake | real], the foreach kernels of the two AdamW / clip_grad_norm_ paths, the reductions (scalar means, norms), elementwise
arithmetic, and the runtime's copy / fill kernels."""
import csv
import sys

FAMILIES = (("torch.cat of [fake | real] (CatArrayBatchedCopy)", ("CatArray",)),
            ("AdamW / clip_grad_norm_ foreach (multi_tensor_apply)", ("multi_tensor_apply",)),
            ("reductions: scalar means, norms, sums (reduce_kernel)", ("reduce_kernel",)),
            ("elementwise arithmetic (elementwise_kernel)", ("elementwise_kernel",)),
            ("runtime copy / fill (__amd_rocclr_*)", ("__amd_rocclr",)))


def family(name):
    if "escx" in name:
        return "libescx"
    for fam, keys in FAMILIES:
        if any(k in name for k in keys):
            return fam
    return "other torch kernels"


def summarise(path, steps, title):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    fam = {}
    for r in rows:
        f = fam.setdefault(family(r["Name"]), [0.0, 0, {}])
        f[0] += float(r["TotalDurationNs"])
        f[1] += int(r["Calls"])
        f[2][r["Name"]] = float(r["TotalDurationNs"])
    print(f"{title}: {steps} steps, kernel time {total / steps / 1e6:.2f} ms per step, {sum(int(r['Calls']) for r in rows) / steps:.0f} launches per step")
    for name, (ns, calls, members) in sorted(fam.items(), key=lambda kv: -kv[1][0]):
        print(f"    {name:58s} {ns / steps / 1e6:9.3f} ms / step  {100 * ns / total:6.2f} %   {calls / steps:7.1f} launches / step")
        if name == "other torch kernels":
            for k, v in sorted(members.items(), key=lambda kv: -kv[1])[:5]:
                print(f"        {k[:120]:120s} {100 * v / total:.2f} %")
    print()


if __name__ == "__main__":
    a = sys.argv[1:]
    for i in range(0, len(a), 3):
        summarise(a[i], float(a[i + 1]), a[i + 2])
