#!/bin/bash
# Is the device code of the working tree the same as at <git-rev>?   tools/isa_diff.sh <git-rev>   (no GPU needed)
# Both trees' shim.hip go to assembly with the flags of libmspack_amd/build.py; the one symbol that names the compilation
# (__hip_cuid_<hash>) is rewritten.  Prints IDENTICAL, or the first differing lines and exits 1.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
mkdir "$T/old" && git -C "$R" archive "${1:?usage: tools/isa_diff.sh <git-rev>}" libmspack_amd/csrc/hip include | tar -x -C "$T/old"
for t in old new; do
  S=$T/old; [ $t = new ] && S=$R
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -I "$S/include" --cuda-device-only -S "$S/libmspack_amd/csrc/hip/shim.hip" -o "$T/$t.raw" 2> "$T/$t.err" &
done
wait    # (a failed compile leaves no output file: checked below)
for t in old new; do
  [ -s "$T/$t.raw" ] || { echo "shim.hip does not compile ($t tree):"; cat "$T/$t.err"; exit 2; }
  sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$T/$t.raw" > "$T/$t.s"
done
if cmp -s "$T/old.s" "$T/new.s"; then echo "IDENTICAL ($(wc -l < "$T/new.s") lines of assembly, $1 vs working tree)"; else diff "$T/old.s" "$T/new.s" | head -40; exit 1; fi
