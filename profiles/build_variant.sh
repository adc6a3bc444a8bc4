#!/bin/bash
# Compile-time A/B variants of one kernel file (a CPU-only build, no device needed):
#   bash profiles/build_variant.sh NAME "-DMACRO=value ..." [SOURCE]
# builds fuzzy_aho_corasick/_lib/libfac_NAME.so from the current sources with the extra flags on
# SOURCE.hip (default search_kernels; prefilter_kernels for the q-gram knobs), the other objects from
# the regular build; select it with FAC_LIB=<that path>.
set -eo pipefail
NAME=${1:?name}
FLAGS=${2:-}
SRC=${3:-search_kernels}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
C=$ROOT/fuzzy-aho-corasick-rs_amd/csrc
make -s -C "$C" >/dev/null
mkdir -p "$C/build/var"
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function \
  --offload-arch=gfx950 -fno-gpu-flush-denormals-to-zero -fno-gpu-rdc $FLAGS -c -o "$C/build/var/${SRC}_$NAME.o" "$C/$SRC.hip"
OTHERS=()  # the regular objects but SOURCE's (NAME_kernels_SUFFIX.o: a side library's own build)
for o in "$C"/build/*.o; do
  case "$o" in "$C/build/$SRC.o" | *_kernels_*.o) ;; *) OTHERS+=("$o") ;; esac
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o "$ROOT/fuzzy-aho-corasick-rs_amd/fuzzy_aho_corasick/_lib/libfac_$NAME.so" \
  "${OTHERS[@]}" "$C/build/var/${SRC}_$NAME.o"
echo "built libfac_$NAME.so"
