# rocprofv3 kernel statistics of one bench workload.  usage (on the GPU box): bash tools/kernel_stats.sh <workload> <tag>   -> $XEVD_OUT/<tag>_<workload>_kernel_stats.csv (default out/)
R=$GRAFT_REPO_ROOT; wl=$1; T=$2
OUT=${XEVD_OUT:-$R/out}; mkdir -p $OUT      # where the outputs go (default: out/ in the repository)
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/kt_$wl
timeout -k 5 200 rocprofv3 --kernel-trace --stats -d $OUT/kt_$wl -o p -- python $R/bench.py --steps 30 --warmup 5 --workload $wl --no-cpu-baseline --no-end-to-end --full > $OUT/kt_$wl.log 2>&1
python $R/tools/rocpd_stats.py $(find $OUT/kt_$wl -name "*.db" | head -1) $OUT/${T}_${wl}_kernel_stats.csv
rm -rf $OUT/kt_$wl
