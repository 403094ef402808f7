#!/bin/bash
# tools/build_variant.sh NAME [extra hipcc flags...]: builds tools/_variants/libcrd_NAME.so (same sources, extra -D flags) for A/B
# timing against the in-tree library (CRD_LIBRARY=tools/_variants/libcrd_NAME.so); the objects go to a private directory.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
OUT=$ROOT/tools/_variants; mkdir -p $OUT/obj_$NAME
cd $ROOT/crdmodel_amd/csrc
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$ROOT/include -I/opt/rocm/include $*"
for f in crd_host.cpp crd_io.cpp crd_context.cpp crd_halo.cpp crd_steppers.cpp crd_adaptive.cpp crd_trace.cpp crd_kernel_table.cpp crd_ensemble.cpp; do /opt/rocm/bin/hipcc $FLAGS -DCRD_NO_KERNEL_TABLE -x hip -c $f -o $OUT/obj_$NAME/${f%.*}.o & done
for f in crd_kernels.hip crd_fused.hip; do /opt/rocm/bin/hipcc $FLAGS -c $f -o $OUT/obj_$NAME/${f%.*}.o & done
/opt/rocm/bin/hipcc $FLAGS -c crd_observe.hip -o $OUT/obj_$NAME/crd_observe.o &
/opt/rocm/bin/hipcc $FLAGS -fno-slp-vectorize -c crd_ensemble.hip -o $OUT/obj_$NAME/crd_ensemble_kernels.o &  # (crd_ensemble.o is the host code's)
for f in crd_ensemble_adaptive crd_ensemble_mixed crd_ensemble_own; do /opt/rocm/bin/hipcc $FLAGS -fno-slp-vectorize -c $f.hip -o $OUT/obj_$NAME/$f.o & done
# (the pair units as the Makefile builds them: their device assembly kept and checked before the link)
for f in crd_ensemble_multi crd_ensemble_mixed_multi; do /opt/rocm/bin/hipcc $FLAGS -fno-slp-vectorize -save-temps=obj -c $f.hip -o $OUT/obj_$NAME/$f.o & done
/opt/rocm/bin/hipcc $FLAGS -fno-slp-vectorize -c crd_fused_f32.hip -o $OUT/obj_$NAME/crd_fused_f32.o &  # (as the Makefile builds it)
wait
for f in crd_ensemble_multi crd_ensemble_mixed_multi; do
  python3 $ROOT/tools/kernel_regs.py --check --asm $OUT/obj_$NAME/$f-hip-amdgcn-amd-amdhsa-gfx950.s > $OUT/obj_$NAME/$f.checked
  rm -f $OUT/obj_$NAME/$f-h*.bc $OUT/obj_$NAME/$f-h*.hipi $OUT/obj_$NAME/$f-hip-*.o $OUT/obj_$NAME/$f-hip-*.out $OUT/obj_$NAME/$f-hip-*.resolution.txt $OUT/obj_$NAME/$f.hip-hip-*.hipfb
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o $OUT/libcrd_$NAME.so $OUT/obj_$NAME/*.o -L/opt/rocm/lib -ldl -lpthread -Wl,-rpath,/opt/rocm/lib
rm -rf $OUT/obj_$NAME
echo $OUT/libcrd_$NAME.so
