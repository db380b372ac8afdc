#!/bin/bash
# gen_build_info.sh OUT.cpp "FLAGS": writes the fw_build_info() translation unit (include/
# flipwalk.h) of a build: a hash over every kernel, header and ABI source plus the flags.
set -e
cd "$(dirname "$0")"
OUT=$1
FLAGS=$2
H=$(cat fw_api.hip fw_kernels.hip fw_grid16.hip fw_grid16_lean.hip fw_grid16_w2.hip fw_internal.h fw_device.h fw_math.h \
      ../../include/flipwalk.h | sha256sum | cut -c1-16)
# the series kernels are hashed on their own: "src" stays the hash of the list above
S=$(cat fw_series.hip | sha256sum | cut -c1-16)
T=$(cat fw_tally.hip | sha256sum | cut -c1-16)
G=$(cat fw_geometry.hip | sha256sum | cut -c1-16)
W=$(cat fw_window_rows.h | sha256sum | cut -c1-16)
O=$(cat fw_overlap.hip fw_overlap_bits.h | sha256sum | cut -c1-16)
R=$(cat fw_resample.hip fw_resample_limbs.h | sha256sum | cut -c1-16)
C=$(cat fw_census.hip fw_census_plan.h | sha256sum | cut -c1-16)
P=$(cat fw_pairdist.hip fw_pairdist_planes.h fw_pairdist_plan.h | sha256sum | cut -c1-16)
A=$(cat fw_coassign.hip fw_coassign_plan.h | sha256sum | cut -c1-16)
B=$(cat fw_weights_bytes.h | sha256sum | cut -c1-16)
printf 'extern "C" const char* fw_build_info(void) { return "src=%s flags=%s series=%s tally=%s geom=%s win=%s ovl=%s rsm=%s wb=%s cen=%s pwd=%s coa=%s"; }\n' \
  "$H" "$(echo $FLAGS)" "$S" "$T" "$G" "$W" "$O" "$R" "$B" "$C" "$P" "$A" > "$OUT.tmp"
# rewrite only on change, so make relinks only when the provenance changes
if ! cmp -s "$OUT.tmp" "$OUT" 2>/dev/null; then mv "$OUT.tmp" "$OUT"; else rm -f "$OUT.tmp"; fi
