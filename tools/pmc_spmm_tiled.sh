#!/bin/bash
# HBM-side traffic of the untiled and the tiled SpMM route on config 3's community_1000_p90 leg (2M x 2M, nnz 40M, D = 256 bf16):
# FETCH_SIZE and WRITE_SIZE in passes of their own per route, summarised by tools/pmc_summarise.py.
# usage (GPU box): bash tools/pmc_spmm_tiled.sh OUTDIR   -> OUTDIR/{untiled,tiled}/{fetch,write}/ (counter CSVs: keep OUTDIR out of git)
root=$(cd "$(dirname "$0")/.." && pwd)
[ -n "$1" ] || { echo "usage: bash tools/pmc_spmm_tiled.sh OUTDIR"; exit 2; }
mkdir -p "$1" && out=$(cd "$1" && pwd)
for route in untiled tiled; do
  mkdir -p $out/$route/fetch $out/$route/write
  for pass in fetch write; do
    ctr=FETCH_SIZE; [ $pass = write ] && ctr=WRITE_SIZE
    timeout -k 10 280 rocprofv3 --pmc $ctr --output-format csv -d $out/$route/$pass -o p -- python3 $root/tools/time_spmm.py --pmc-workload community_1000_p90:$route > $out/$route/$pass/stdout.log 2> $out/$route/$pass/err.log
    rc=$?
    echo "$route $pass exit $rc"
    [ $rc = 0 ] || { tail -5 $out/$route/$pass/err.log; exit $rc; }
  done
  echo "== $route"
  python3 $root/tools/pmc_summarise.py $out/$route | grep -i spmm
done
