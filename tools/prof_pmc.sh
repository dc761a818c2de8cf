# usage: prof_pmc.sh <tag> <workload> "<counters>"   -> $XEVD_OUT/<tag>.csv (default out/; one --pmc pass, no other tracing)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${XEVD_OUT:-$R/out}; mkdir -p $OUT      # where the outputs go (default: out/ in the repository)
rm -rf $OUT/pmc_$1
timeout -k 5 150 rocprofv3 --pmc $3 -d $OUT/pmc_$1 -o p -- python $R/bench.py --steps 6 --warmup 2 --workload $2 --no-cpu-baseline --no-end-to-end --full > $OUT/pmc_$1.log 2>&1
python $R/tools/rocpd_pmc.py $(find $OUT/pmc_$1 -name "*.db" | head -1) $OUT/$1.csv | cut -c1-150 | head -40
rm -rf $OUT/pmc_$1
