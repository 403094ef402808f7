#!/usr/bin/env python3
"""Registers, LDS, scratch and wavefronts per SIMD of the kernels of crd_jacobian.hip, beside crd_rhs_aos_kernel's.

    tools/jacobian_resources.py > profiles/jacobian/kernel_resources.txt

Reads the device assembly the build keeps for crd_jacobian.hip (crdmodel_amd/csrc/Makefile: -save-temps=obj) and compiles
crd_kernels.hip to assembly for the comparison rows (tools/kernel_regs.py: compile_to_asm).  No GPU needed.  Exit 1 if a kernel of
crd_jacobian.hip has scratch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs as kr  # noqa: E402

CSRC = os.path.join(kr.ROOT, "crdmodel_amd", "csrc")
ASM = os.path.join(CSRC, "build", "crd_jacobian-hip-amdgcn-amd-amdhsa-gfx950.s")


def rows(kernels, keep):
    out = []
    for k in kernels:
        if keep(k["name"]):
            out.append("%-78s %5d %5d %6d %7d %5d" % (k["name"], k["vgprs"], k["sgprs"], k["lds"], k["scratch"], k["occupancy"]))
    return sorted(out)


def main():
    if not os.path.exists(ASM):
        sys.exit("build the library first: %s is not there" % ASM)
    jac = kr.parse(open(ASM).read())
    ref = kr.parse(kr.compile_to_asm(os.path.join(CSRC, "crd_kernels.hip"), []))
    print("# tools/jacobian_resources.py: gfx950, read from the build's device assembly.  Template arguments: <Real, MODEL, PART, NT>;")
    print("# MODEL 0 FHN, 1 Goldbeter, 2 diffusion only; PART 0 full, 1 diffusion, 2 reaction; NT: non-temporal stores.  Blocks of 256 threads.")
    print("%-78s %5s %5s %6s %7s %5s" % ("# kernel", "VGPR", "SGPR", "LDS B", "scratch", "w/SIMD"))
    for ln in rows(jac, lambda n: n.startswith(("crd_rhs_part_aos_kernel", "crd_jtimes_aos_kernel"))):
        print(ln)
    print("# for comparison (crd_kernels.hip, same flags): <Real, MODEL, NT>")
    for ln in rows(ref, lambda n: n.startswith("crd_rhs_aos_kernel")):
        print(ln)
    bad = [k["name"] for k in jac if k["scratch"]]
    if bad:
        sys.exit("scratch in: " + ", ".join(bad))


if __name__ == "__main__":
    main()
