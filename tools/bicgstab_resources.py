#!/usr/bin/env python3
"""Registers, LDS, scratch and wavefronts per SIMD of the kernels of crd_bicgstab.hip.

    tools/bicgstab_resources.py > profiles/bicgstab/kernel_resources.txt

Reads the device assembly the build keeps for crd_bicgstab.hip (crdmodel_amd/csrc/Makefile: -save-temps=obj).  No GPU needed.
Exit 1 if a kernel has scratch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs as kr  # noqa: E402

ASM = os.path.join(kr.ROOT, "crdmodel_amd", "csrc", "build", "crd_bicgstab-hip-amdgcn-amd-amdhsa-gfx950.s")


def main():
    if not os.path.exists(ASM):
        sys.exit("build the library first: %s is not there" % ASM)
    kernels = [k for k in kr.parse(open(ASM).read()) if k["name"].startswith("crd_bcg_")]
    print("# tools/bicgstab_resources.py: gfx950, read from the build's device assembly.  Template arguments: <Real> (apply-dot: <Real, two dots>).")
    print("# Blocks of 256 threads; crd_bcg_sum_kernel: one wavefront.")
    print("%-44s %5s %5s %6s %7s %5s" % ("# kernel", "VGPR", "SGPR", "LDS B", "scratch", "w/SIMD"))
    for ln in sorted("%-44s %5d %5d %6d %7d %5d" % (k["name"], k["vgprs"], k["sgprs"], k["lds"], k["scratch"], k["occupancy"]) for k in kernels):
        print(ln)
    if len(kernels) != 15:
        sys.exit("expected seven templated kernels in two precisions (apply-dot twice) and the partials' sum, found %d" % len(kernels))
    bad = [k["name"] for k in kernels if k["scratch"]]
    if bad:
        sys.exit("scratch in: " + ", ".join(bad))


if __name__ == "__main__":
    main()
