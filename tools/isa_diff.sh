#!/bin/bash
# Do two builds hold the same gfx950 instructions?  For every *.o present in both directories: unbundle the gfx950 code object
# (as tools/kernel_resources.sh does), disassemble it and diff.  The __hip_cuid_* symbol (a hash of the source TEXT) is ignored;
# the host half of the objects is not compared.  Exit status 1 on any difference or on an object that only one side has.
# usage: bash tools/isa_diff.sh <dir of objects A> <dir of objects B>
set -u
B=/opt/rocm/lib/llvm/bin
T=$(mktemp -d); trap 'rm -rf $T' EXIT
isa() {  # <object> <output>; fails when the object holds no gfx950 code (host-only objects)
  $B/llvm-objcopy --dump-section .hip_fatbin=$T/fb.bin $1 2>/dev/null &&
    $B/clang-offload-bundler --unbundle --type=o --input=$T/fb.bin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$T/k.co 2>/dev/null &&
    $B/llvm-objdump -d $T/k.co | grep -v -e __hip_cuid_ -e 'file format' > $2
}
bad=0; n=0
for name in $( (cd $1 && ls *.o; cd $2 && ls *.o) 2>/dev/null | sort -u); do
  if [ ! -f $1/$name ] || [ ! -f $2/$name ]; then echo "$name: only on one side"; bad=1; continue; fi
  isa $1/$name $T/a.s; ra=$?; isa $2/$name $T/b.s; rb=$?
  if [ $ra != 0 ] && [ $rb != 0 ]; then continue; fi   # no device code on either side
  if [ $ra != $rb ]; then echo "$name: device code on one side only"; bad=1; continue; fi
  n=$((n + 1))
  if ! diff -q $T/a.s $T/b.s > /dev/null; then echo "$name: DIFFERENT ($(wc -l < $T/a.s) / $(wc -l < $T/b.s) lines)"; diff $T/a.s $T/b.s | head -20; bad=1; fi
done
echo "$n objects with gfx950 code compared: $([ $bad = 0 ] && echo identical || echo DIFFERENCES)"
exit $bad
