#!/usr/bin/env python3
"""Registers, LDS, scratch and wavefronts per SIMD of the kernels of crd_imex.hip.

    tools/imex_resources.py > profiles/imex/kernel_resources.txt

Reads the device assembly the build keeps for crd_imex.hip (crdmodel_amd/csrc/Makefile: -save-temps=obj).  No GPU needed.
Exit 1 if a kernel has scratch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs as kr  # noqa: E402

ASM = os.path.join(kr.ROOT, "crdmodel_amd", "csrc", "build", "crd_imex-hip-amdgcn-amd-amdhsa-gfx950.s")


def main():
    if not os.path.exists(ASM):
        sys.exit("build the library first: %s is not there" % ASM)
    kernels = [k for k in kr.parse(open(ASM).read()) if k["name"].startswith("crd_imex_")]
    print("# tools/imex_resources.py: gfx950, read from the build's device assembly.  Template arguments of the stage close: <Real, model (0 FHN, 1 Goldbeter,")
    print("# 2 Goldbeter with diffusion only), last stage>.  Blocks of 256 threads; crd_imex_max_kernel, crd_imex_max_sum_kernel: one wavefront.")
    print("%-48s %5s %5s %6s %7s %5s" % ("# kernel", "VGPR", "SGPR", "LDS B", "scratch", "w/SIMD"))
    for ln in sorted("%-48s %5d %5d %6d %7d %5d" % (k["name"], k["vgprs"], k["sgprs"], k["lds"], k["scratch"], k["occupancy"]) for k in kernels):
        print(ln)
    if len(kernels) != 16:
        sys.exit("expected the stage close for three models, two precisions, last stage or not, the partials' maximum, the estimating close for two "
                 "precisions and its partials' maximum and sum, found %d" % len(kernels))
    bad = [k["name"] for k in kernels if k["scratch"]]
    if bad:
        sys.exit("scratch in: " + ", ".join(bad))


if __name__ == "__main__":
    main()
