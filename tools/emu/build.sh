#!/bin/sh
# Builds tools/emu/build/libsemseg_emu.so: the UNCHANGED kernel sources of semantic-segmentation_amd/csrc compiled
# for the host against the CPU emulation shim (tools/emu/include).  Test infrastructure only.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
SRC="$ROOT/semantic-segmentation_amd/csrc"
# sh tools/emu/build.sh f16 : the fp16-storage build (-DSSA_ELEM_F16) -> build_f16/libsemseg_emu.so
if [ "$1" = "f16" ]; then OUT="$HERE/build_f16"; EXTRA="-DSSA_ELEM_F16"; else OUT="$HERE/build"; EXTRA=""; fi
CXX=${EMU_CXX:-/opt/rocm/lib/llvm/bin/clang++}
FLAGS="-x c++ -std=c++17 -O2 -g0 -fPIC -DSSA_EMU $EXTRA -I$HERE/include -Wno-unused-function -Wno-unused-value -Wno-unknown-pragmas -Wno-pass-failed"
mkdir -p "$OUT"
pids=""
objs=""
for f in "$SRC"/*.hip "$HERE/emu_runtime.cpp"; do
  o="$OUT/$(basename "$f" | sed 's/\.[a-z]*$//').o"
  objs="$objs $o"
  for d in "$f" "$SRC"/*.h "$HERE/include/hip/hip_runtime.h" "$ROOT/include/semseg_hip.h"; do
    if [ ! -f "$o" ] || [ "$d" -nt "$o" ]; then
      $CXX $FLAGS -c "$f" -o "$o" &
      pids="$pids $!"
      break
    fi
  done
done
for p in $pids; do wait "$p"; done
# Several processes may run this at once (every rank of a multi-process test calls it) while others already have the
# library loaded or are about to load it.  So: relink only when an object is newer than the library, and link to a
# temporary name that is renamed into place -- the linker removes its output file before writing it, and a process
# that opened the library in that window found no file.
LIB="$OUT/libsemseg_emu.so"
relink=0
[ -f "$LIB" ] || relink=1
for o in $objs; do if [ "$o" -nt "$LIB" ]; then relink=1; fi; done
if [ "$relink" = 1 ]; then
  tmp="$LIB.tmp.$$"
  $CXX -shared -fPIC -o "$tmp" $objs -lpthread || { rm -f "$tmp"; exit 1; }
  mv -f "$tmp" "$LIB"
fi
echo "built $LIB"
