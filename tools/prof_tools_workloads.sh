# rocprofv3 kernel stats of the two Main-tool workloads outside BASELINE's configs (affine, HTDF).  usage (through gpurun): bash tools/prof_tools_workloads.sh <tag>
R=$GRAFT_REPO_ROOT; T=$1
OUT=${XEVD_OUT:-$R/out}; mkdir -p $OUT      # where the outputs go (default: out/ in the repository)
cd /tmp && export TMPDIR=/tmp
for wl in main_8k_10b_ra_affine30 main_8k_10b_ra_htdf; do
  rm -rf $OUT/kt_$wl
  timeout -k 5 200 rocprofv3 --kernel-trace --stats -d $OUT/kt_$wl -o p -- python $R/bench.py --steps 20 --warmup 5 --workload $wl --no-cpu-baseline --full > $OUT/kt_$wl.log 2>&1
  python $R/tools/rocpd_stats.py $(find $OUT/kt_$wl -name "*.db" | head -1) $OUT/${T}_${wl}_kernel_stats.csv > /dev/null
  rm -rf $OUT/kt_$wl
done
ls -la $OUT | grep ${T}_main_8k
