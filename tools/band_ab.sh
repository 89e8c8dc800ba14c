#!/bin/bash
# The band-launch measurements of EXPERIMENTS.md "Tile-band launches" (tools/band_ab.py has the method): the whole
# C3 frame as render_jobs vs render_tiles(0, T), the emulated strong-scaling shares, and the write counters of one
# launch of each kind -- rocprofv3 --pmc alone, no tracing, one pass per counter group.  Every step runs under its own
# time limit and the first failure ends the script.  Logs: $OUT_DIR/<tag>/ (default bench_outputs/; copy them to profiles/).
# Usage (GPU box): bash tools/band_ab.sh <tag> [config] [frame|shares|pmc ...]
set -u
TAG=${1:-bands}; CFG=${2:-c3}; shift 2 || shift $#
STEPS=${*:-frame shares pmc}
O=${OUT_DIR:-bench_outputs}/$TAG; mkdir -p $O; export TMPDIR=/tmp
step() { local name=$1 to=$2; shift 2; echo "== $name"; timeout -k 10 "$to" "$@" > $O/$name.log 2>&1; local rc=$?; echo "== $name rc=$rc"; tail -1 $O/$name.log | cut -c1-1500; if [ $rc -ne 0 ]; then tail -5 $O/$name.log; exit $rc; fi; }
for S in $STEPS; do
  case $S in
    frame) step ${CFG}_frame 240 python3 tools/band_ab.py frame --config $CFG ;;
    shares) step ${CFG}_shares 300 python3 tools/band_ab.py shares --config $CFG ;;
    pmc)
      for KIND in jobs tiles; do
        i=0
        for P in "TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum" "WRITE_SIZE"; do
          i=$((i+1))
          step ${CFG}_pmc_${KIND}_$i 240 rocprofv3 --pmc $P --output-format csv -d $O/${CFG}_pmc_${KIND}_$i -o run -- python3 tools/band_ab.py one --kind $KIND --config $CFG
        done
        step ${CFG}_pmc_${KIND} 60 python3 tools/band_ab.py pmc $O/${CFG}_pmc_${KIND}_1 $O/${CFG}_pmc_${KIND}_2
      done ;;
    *) echo "unknown step $S"; exit 2 ;;
  esac
done
