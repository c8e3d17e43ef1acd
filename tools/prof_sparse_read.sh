#!/bin/bash
# usage: tools/prof_sparse_read.sh [GiB] -- tools/probe/sparse_read (built beforehand) once for its rates, then once under the
# FETCH_SIZE PMC pass of tools/prof_traffic.sh (a run of its own, one launch per pattern and phase); per kernel: FETCH_SIZE per
# dispatch in bytes, doubled as tools/prof_summary.py doubles it, and per 254-byte period.  Output: $FG_RESULTS/sparse_read.log (default results/)
ROOT=$(pwd)
GIB=${1:-4}
OUT=/tmp/sparse_read_pmc
RES=$ROOT/${FG_RESULTS:-results}
rm -rf $OUT; mkdir -p $OUT $RES
LOG=$RES/sparse_read.log
timeout -k 10 200 $ROOT/tools/probe/sparse_read $GIB 4 > $LOG 2>&1 || { echo "probe failed: $?" >> $LOG; tail -5 $LOG; exit 1; }
cd /tmp && export TMPDIR=/tmp
timeout -k 10 280 rocprofv3 --kernel-trace --output-format csv --pmc FETCH_SIZE -d $OUT -o pmc -- $ROOT/tools/probe/sparse_read $GIB 1 > $OUT/pmc.log 2>&1 \
    || { echo "pmc pass failed: $?" >> $LOG; tail -5 $OUT/pmc.log >> $LOG; cat $LOG; exit 1; }
cd $ROOT
python - $OUT $GIB >> $LOG <<'PY'
import csv, glob, os, sys
d, gib = sys.argv[1], int(sys.argv[2])
swept = (gib << 30) // 20480 * 20480
print("FETCH_SIZE per dispatch (launch order; doubled = 2 x FETCH_SIZE x 1024 B)")
for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
    rows = [r for r in csv.DictReader(open(f)) if "k_read" in r.get("Kernel_Name", "") and r["Counter_Name"] == "FETCH_SIZE"]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        b = float(r["Counter_Value"]) * 1024
        print("%-28s raw %8.1f MB  doubled %8.1f MB  per period raw %6.1f doubled %6.1f" %
              (r["Kernel_Name"][:28], b / 1e6, 2 * b / 1e6, b / swept * 254, 2 * b / swept * 254))
PY
cat $LOG
