# usage: prof_kt.sh <workload>  -> per-kernel stats of a short bench run (rocprofv3 --kernel-trace)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${XEVD_OUT:-$R/out}; mkdir -p $OUT      # where the outputs go (default: out/ in the repository)
rm -rf $OUT/kt
timeout -k 5 200 rocprofv3 --kernel-trace --stats -d $OUT/kt -o p -- python $R/bench.py --steps 30 --warmup 5 --workload $1 --no-cpu-baseline --full > $OUT/kt.log 2>&1
python $R/tools/rocpd_stats.py $(find $OUT/kt -name "*.db" | head -1) | cut -c1-110
rm -rf $OUT/kt
