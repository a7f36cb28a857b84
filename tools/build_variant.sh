# usage: bash tools/build_variant.sh <name> <extra hipcc flags...>   -> ab/libsynthray_<name>.so (trace.hip rebuilt with the flags,
# linked with every other object of the Makefile's SRC)
set -e
R=$(cd "$(dirname "$0")/.." && pwd); name=$1; shift
C=$R/synthpy_amd/csrc
make -s -j8 -C $C
mkdir -p $R/ab
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -munsafe-fp-atomics -I$R/include -Wall -Wno-unused-function "$@" -c $C/trace.hip -o /tmp/trace_$name.o
objs=""
for s in $(sed -n 's/^SRC *= *//p' $C/Makefile); do
  if [ $s = trace.hip ]; then objs="$objs /tmp/trace_$name.o"; else objs="$objs ${s%.hip}.o"; fi
done
cd $C && /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o $R/ab/libsynthray_$name.so $objs -ldl
echo built ab/libsynthray_$name.so
