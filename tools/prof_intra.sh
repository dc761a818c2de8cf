cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${XEVD_OUT:-$R/out}; mkdir -p $OUT      # where the outputs go (default: out/ in the repository)
rocprofv3 --kernel-trace --stats -d $OUT/prof_intra -o p -- python $R/bench.py --steps 30 --warmup 5 --workload cfg2_base_1080p_8b_ippp --no-cpu-baseline --full > $OUT/prof_intra.log 2>&1
find $OUT/prof_intra -name "*.db" | head -3
python $R/tools/rocpd_stats.py $(find $OUT/prof_intra -name "*.db" | head -1) 2>&1 | cut -c1-160 | head -30
