#!/bin/bash
# The verify mode's measurements on one box (DESIGN §4.4 "Verify", profiles/flac_verify_*):
#     tools/flac_verify_profile.sh <out dir> <parent lib.so>
# Wall clocks of sauAmd_render_file_flac_lpc (16 bits) and sauAmd_render_file_flac_lpc24, max_lpc_order 8, on
# examples__rainy_thunder at 44100 Hz stereo, B = 4096, three renders a process, by turns: (a) the parent commit's library
# (`tools/ab_variant.sh HEAD~1 parent`), (b) this one with verify off, (c) with verify on -- twice, so that (a)'s spread from run
# to run is on record. Then kernel statistics (rocprofv3 --kernel-trace --stats, no counters, a pass of its own per setting) of
# (a), (b) and (c) at both widths, and the kernel's time by kind of frame (tools/flac_verify_split.py). Every step under a time
# limit of its own; the first that fails ends the script.
set -e -o pipefail
OUT=$1; PARENT=$2
mkdir -p "$OUT"
for rep in 1 2; do
  for bits in 16 24; do
    SAU_AMD_LIB=$PARENT timeout -k 10 120 python3 tools/flac_verify_measure.py $bits 0 3 "$OUT/flac_verify_ab.jsonl" | tail -1
    timeout -k 10 120 python3 tools/flac_verify_measure.py $bits 0 3 "$OUT/flac_verify_ab.jsonl" | tail -1
    timeout -k 10 120 python3 tools/flac_verify_measure.py $bits 1 3 "$OUT/flac_verify_ab.jsonl" | tail -1
  done
done
for v in parent:0 off:0 on:1; do
  name=${v%%:*}; on=${v##*:}; lib=""
  [ "$name" = parent ] && lib=$PARENT
  for bits in 16 24; do
    SAU_AMD_LIB=$lib timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_${name}_$bits" -o s -- \
      python3 tools/flac_verify_measure.py $bits $on 3 > "$OUT/prof_${name}_$bits.log" 2>&1
    cp "$OUT"/prof_${name}_$bits/*/s_kernel_stats.csv "$OUT/flac_verify_${name}_${bits}_kernel_stats.csv" 2>/dev/null || \
      cp "$OUT"/prof_${name}_$bits/s_kernel_stats.csv "$OUT/flac_verify_${name}_${bits}_kernel_stats.csv"
    tail -1 "$OUT/prof_${name}_$bits.log"
  done
done
# where the decode kernel's time goes: single frames of one kind each, a workgroup a launch (tools/flac_verify_split.py)
timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d "$OUT/split" -o s -- \
  python3 tools/flac_verify_split.py "$OUT/flac_verify_split.jsonl" > "$OUT/split.log" 2>&1
TRACE=$(ls "$OUT"/split/*/s_kernel_trace.csv "$OUT"/split/s_kernel_trace.csv 2>/dev/null | head -1 || true)
python3 tools/flac_verify_split.py --summary "$TRACE" "$OUT/flac_verify_split.jsonl" > "$OUT/flac_verify_split_us.csv"
tail -3 "$OUT/flac_verify_split_us.csv"
