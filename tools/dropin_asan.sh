#!/bin/bash
# Builds the host code of the drop-in calls for device-resident arrays (sz_api.c and the rest of the C layer) and the HIP layer over the HIP-on-CPU shim
# (tests/sim) with AddressSanitizer + UndefinedBehaviorSanitizer into ONE stand-alone program (tools/dropin_asan.c) and runs it.  Host code on the CPU only.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
CSRC="$ROOT/sz_amd/csrc"; SIM="$ROOT/tests/sim"
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer -g -O1"
CF="$SAN -std=gnu99 -ffp-contract=off -fno-fast-math -I$ROOT/include"
for f in szhost sz_api sz_conf sz_rw sz_slab; do gcc $CF -Wno-int-in-bool-context -c "$CSRC/$f.c" -o "$OUT/$f.o"; done
gcc $CF -c "$ROOT/tools/dropin_asan.c" -o "$OUT/dropin_asan.o"
CXXF="$SAN -std=c++17 -ffp-contract=off -fno-fast-math -w"
g++ $CXXF -x c++ -I"$SIM/hip_shim" -I"$CSRC" -c "$SIM/hipsim.cpp" -o "$OUT/hipsim.o"
g++ $CXXF -I"$SIM/hip_shim" -I"$ROOT/include" -c "$CSRC/sz_slab_multi.cpp" -o "$OUT/sz_slab_multi.o"
g++ $SAN -o "$OUT/dropin_asan" "$OUT"/*.o -lpthread -ldl -lm
"$OUT/dropin_asan"
