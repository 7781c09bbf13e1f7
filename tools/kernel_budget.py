#!/usr/bin/env python
"""Register / LDS budget of the kernels that share a CU in the lock-step: needs hipcc, no GPU.

Two convolution workgroups are resident per CU: 2 waves x 240 VGPRs of a SIMD's 512 and 2 x 64..70 KB of the CU's 160 KB of LDS.  A
step kernel's 256-thread workgroup (one wave per SIMD) fits beside them with <= 32 VGPRs and <= 16 KB of LDS.  This tool compiles the
step's files and nbp_split.hip for gfx950 with -Rpass-analysis=kernel-resource-usage, prints allocated VGPRs (granule 8), scratch and
static LDS of the step's group kernels and of the inference instantiations of conv3x3_halo_h2_kernel, and exits non-zero when
  * a step kernel that was brought inside the budget leaves it (GUARDED), or
  * an inference convolution instantiation allocates more than 240 VGPRs.
    python tools/kernel_budget.py [--out profiles/r08/kernel_budget.txt]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextbestpath_amd import build as nbuild  # noqa: E402

STEP_FILES = ("nbp_sim.hip", "nbp_planner.hip", "nbp_maps.hip")
STEP_VGPRS, STEP_LDS, CONV_VGPRS = 32, 16 * 1024, 240
# the group kernels held to the budget (the others are printed for the record)
GUARDED = ("raster_tile_batch_kernel", "raster_setup_batch_kernel", "coverage_mark_batch_kernel<4, 4>", "unproject_append_batch_kernel<false>")


def resource_usage(src):
    """{demangled kernel name: dict(vgprs, agprs, scratch, lds)} of one source file (device code only)."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [nbuild._hipcc(), *nbuild.FLAGS, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
               os.path.join(tmp, "out.o")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.exit(f"hipcc failed on {src}:\n{r.stderr[-4000:]}")
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgprs", r"remark:\s+VGPRs: (\d+)"), ("agprs", r"remark:\s+AGPRs: (\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    names = list(rows)
    dem = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    return {short(d): rows[n] for n, d in zip(names, dem)}


def short(name):
    name = name.replace("void ", "").replace("(anonymous namespace)::", "")
    return name[:name.index("(")] if "(" in name else name


def alloc(v):
    return (v + 7) // 8 * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines, bad = [], []
    lines.append(f"step kernels (group forms; budget: <= {STEP_VGPRS} VGPRs, 0 AGPRs, 0 scratch, <= {STEP_LDS} B of LDS, 256 threads)")
    lines.append(f"{'kernel':72s} {'VGPRs':>6s} {'alloc':>6s} {'scratch':>8s} {'LDS B':>7s}  fits  guarded")
    seen = set()
    for f in STEP_FILES:
        for name, r in sorted(resource_usage(os.path.join(nbuild.CSRC, f)).items()):
            if "_batch_kernel" not in name:
                continue
            fits = r["vgprs"] <= STEP_VGPRS and r.get("agprs", 0) == 0 and r["scratch"] == 0 and r["lds"] <= STEP_LDS
            guarded = name in GUARDED
            seen.add(name)
            lines.append(f"{name:72s} {r['vgprs']:6d} {alloc(r['vgprs']):6d} {r['scratch']:8d} {r['lds']:7d}  {'yes' if fits else 'no ':3s}   {'yes' if guarded else ''}")
            if guarded and not fits:
                bad.append(f"{name} left the step budget: {r}")
    bad += [f"{g}: no such kernel (renamed?)" for g in GUARDED if g not in seen]
    lines.append("")
    lines.append(f"inference instantiations of conv3x3_halo_h2_kernel<FIN, ONE, TW, TM, TN, PH, BS, P2, DG> (two-piece, no batch statistics, no data gradient; "
                 f"limit: {CONV_VGPRS} allocated)")
    lines.append(f"{'instantiation':72s} {'VGPRs':>6s} {'alloc':>6s} {'scratch':>8s} {'LDS B':>7s}")
    n_conv = 0
    for name, r in sorted(resource_usage(os.path.join(nbuild.CSRC, "nbp_split.hip")).items()):
        # <FIN, ONE, TW, TM, TN, PH, BS, P2, DG>: FIN = the launch that finishes a split-K sum, an inference form like the plain one
        m = re.match(r"conv3x3_halo_h2_kernel<(\w+), (\w+), (\d+), (\d+), (\d+), (\w+), (\w+), (\w+), (\w+)>", name)
        if not m or m.group(2) != "false" or m.group(7) != "false" or m.group(9) != "false":
            continue
        n_conv += 1
        total = r["vgprs"] + r.get("agprs", 0)
        lines.append(f"{name:72s} {total:6d} {alloc(total):6d} {r['scratch']:8d} {r['lds']:7d}")
        if alloc(total) > CONV_VGPRS:
            bad.append(f"{name} allocates {alloc(total)} > {CONV_VGPRS} registers: two of its waves leave no room for a step kernel's wave")
    if n_conv == 0:
        bad.append("no inference instantiation of conv3x3_halo_h2_kernel found")
    lines.append("")
    lines.append(f"rule per SIMD: 2 x {CONV_VGPRS} + {STEP_VGPRS} = {2 * CONV_VGPRS + STEP_VGPRS} of 512 registers; per CU: 2 x 70 KB + 16 KB = 156 of 160 KB of LDS")
    lines += ["VIOLATION: " + b for b in bad] or ["ok"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
