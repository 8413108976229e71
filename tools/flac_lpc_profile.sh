#!/bin/bash
# The LPC mode's measurements on one box (profiles/flac_lpc_*):  tools/flac_lpc_profile.sh <out dir> <parent lib.so>
# <parent lib.so> is the parent commit's library, as `tools/ab_variant.sh HEAD~1 parent` builds it
# (saugns_amd/variants/lib_parent.so). tools/ab_run.sh drives bench.py, which has no FLAC path: hence a command set of its own.
# Kernel statistics (rocprofv3 --kernel-trace --stats, no counters) of three renders of each workload, runs alternated: the
# parent commit's library, this tree at max_lpc_order 0, the parent again, this tree at 0 again, this tree at 8. Then wall
# times without the profiler, six renders a process, alternated the same way, twice. Every step under a time limit of its
# own; the first that fails ends the script.
set -e -o pipefail
OUT=$1; PARENT=$2
mkdir -p "$OUT"
for w in rainy config3; do
  i=0
  for v in parent:0 cur:0 parent:0 cur:0 cur:8; do
    i=$((i + 1)); name=${v%%:*}; m=${v##*:}
    if [ "$name" = parent ]; then lib=$PARENT; else lib=""; fi
    SAU_AMD_LIB=$lib timeout -k 10 150 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_${w}_${i}_${name}_m$m" -o s -- \
      python3 tools/flac_lpc_measure.py $w $m 3 > "$OUT/prof_${w}_${i}_${name}_m$m.log" 2>&1
    cp "$OUT"/prof_${w}_${i}_${name}_m$m/*/s_kernel_stats.csv "$OUT/flac_lpc_${w}_${i}_${name}_m${m}_kernel_stats.csv" 2>/dev/null || \
      cp "$OUT"/prof_${w}_${i}_${name}_m$m/s_kernel_stats.csv "$OUT/flac_lpc_${w}_${i}_${name}_m${m}_kernel_stats.csv"
    echo "kernel stats: $w $name m=$m"
  done
done
for rep in 1 2; do
  for w in rainy config3; do
    for v in parent:0 cur:0 cur:8; do
      name=${v%%:*}; m=${v##*:}
      if [ "$name" = parent ]; then lib=$PARENT; else lib=""; fi
      SAU_AMD_LIB=$lib timeout -k 10 120 python3 tools/flac_lpc_measure.py $w $m 6 "$OUT/flac_lpc_wall.jsonl" | tail -1
    done
  done
done
