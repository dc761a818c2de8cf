R=$GRAFT_REPO_ROOT
OUT=${XEVD_OUT:-$R/out}; mkdir -p $OUT      # where the outputs go (default: out/ in the repository)
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/kt_tr
timeout -k 5 200 rocprofv3 --kernel-trace --output-format csv -d $OUT/kt_tr -o p -- python $R/bench.py --steps 12 --warmup 3 --workload cfg4_main_8k_10b_ra --no-cpu-baseline --no-end-to-end --full > $OUT/kt_tr.log 2>&1
f=$(find $OUT/kt_tr -name "*kernel_trace.csv" | head -1)
python - "$f" $OUT/trace_window.txt <<'PY'
import csv,sys
rows=list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r:int(r["Start_Timestamp"]))
# print a window in the middle of the timed region (with prepare): rows 200..260
t0=int(rows[0]["Start_Timestamp"])
out=open(sys.argv[2],"w")
for r in rows:
    out.write("%10.1f %10.1f %8.1f q=%s %s\n"%((int(r["Start_Timestamp"])-t0)/1e3,(int(r["End_Timestamp"])-t0)/1e3,(int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3,r.get("Queue_Id","?"),r["Kernel_Name"][:40]))
PY
rm -rf $OUT/kt_tr
