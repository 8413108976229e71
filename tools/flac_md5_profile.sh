#!/bin/bash
# The MD5's measurements on one box (DESIGN §4.4 "MD5", profiles/flac_md5_*):  tools/flac_md5_profile.sh <out dir> [parent lib.so]
# Kernel statistics (rocprofv3 --kernel-trace --stats, no counters), one run per setting: the single-stream writer on
# examples__rainy_thunder with the switch off and on, a fed encoder of 64 rows with MD5 off and on, and -- with the parent
# commit's library, as `tools/ab_variant.sh HEAD~1 parent` builds it -- the writer on that library, whose kernel list the
# switch-off run has to equal. Every step under a time limit of its own; the first that fails ends the script.
set -e -o pipefail
OUT=$1; PARENT=$2
mkdir -p "$OUT"
run() { # <name> <lib or ""> <measure arguments>
  local name=$1 lib=$2; shift 2
  SAU_AMD_LIB=$lib timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$name" -o s -- \
    python3 tools/flac_md5_measure.py "$@" > "$OUT/prof_$name.log" 2>&1
  cp "$OUT"/prof_$name/*/s_kernel_stats.csv "$OUT/flac_md5_${name}_kernel_stats.csv" 2>/dev/null || \
    cp "$OUT"/prof_$name/s_kernel_stats.csv "$OUT/flac_md5_${name}_kernel_stats.csv"
  tail -1 "$OUT/prof_$name.log"
}
if [ -n "$PARENT" ]; then run parent_writer "$PARENT" writer 0 3; fi
run off_writer "" writer 0 3
run on_writer "" writer 1 3
run off_fed "" fed 0 4
run on_fed "" fed 1 4
