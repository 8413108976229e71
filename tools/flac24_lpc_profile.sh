#!/bin/bash
# The 24-bit LPC mode's measurements on one box (DESIGN §4.4 "LPC at 24 bits", profiles/flac24_lpc_*):
#     tools/flac24_lpc_profile.sh <out dir> [parent lib.so [second parent lib.so]]
# The file sizes of examples__rainy_thunder at 24 bits with max_lpc_order 0, 4 and 8; kernel statistics (rocprofv3
# --kernel-trace --stats, no counters, a pass of its own per setting) of three feeds of config 3's row at 24 and at 16 bits with
# max_lpc_order 0 and 8; then, with the parent commit's library (`tools/ab_variant.sh HEAD~1 parent`) and a second build of the
# same sources, whose spread is the margin, wall times of a 24-bit feed of order 0 and a 16-bit feed of order 8 by turns, twice.
# Every step under a time limit of its own; the first that fails ends the script.
set -e -o pipefail
OUT=$1; PARENT=$2; PARENT2=$3
mkdir -p "$OUT"
timeout -k 10 240 python3 tools/flac24_lpc_measure.py sizes "$OUT/flac24_lpc_sizes.jsonl" | tail -1
for v in 24:0 24:8 16:0 16:8; do
  bits=${v%%:*}; m=${v##*:}; name=b${bits}_m$m
  timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$name" -o s -- \
    python3 tools/flac24_lpc_measure.py feed $bits $m 3 > "$OUT/prof_$name.log" 2>&1
  cp "$OUT"/prof_$name/*/s_kernel_stats.csv "$OUT/flac24_lpc_${name}_kernel_stats.csv" 2>/dev/null || \
    cp "$OUT"/prof_$name/s_kernel_stats.csv "$OUT/flac24_lpc_${name}_kernel_stats.csv"
  tail -1 "$OUT/prof_$name.log"
done
if [ -n "$PARENT" ]; then
  for rep in 1 2; do
    for lib in "$PARENT" "$PARENT2" ""; do
      for v in 24:0 16:8; do
        SAU_AMD_LIB=$lib timeout -k 10 120 python3 tools/flac24_lpc_measure.py feed ${v%%:*} ${v##*:} 6 "$OUT/flac24_lpc_ab.jsonl" | tail -1
      done
    done
  done
fi
