# round evidence: the official bench line (with cpu_baseline), the rocprofv3 kernel stats of the same command,
# and the other architectures' bench lines
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
O=${1:?usage: bash tools/prof_round.sh <output directory>}
mkdir -p $O
timeout 300 python bench.py --full --steps 5 --warmup 2 > $O/bench_r1.json 2> $O/bench_r1.err
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_r1 -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/prof_bench.log 2>&1
timeout 200 python bench.py --full --arch large --steps 3 --warmup 1 --no-cpu-baseline > $O/bench_r1_large.json 2>/dev/null
timeout 200 python bench.py --full --arch huge --steps 3 --warmup 1 --no-cpu-baseline > $O/bench_r1_huge.json 2>/dev/null
find $O/prof_r1 -name "*kernel_stats.csv" | head -3
