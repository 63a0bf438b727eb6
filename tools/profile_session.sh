# Collects the evidence kept under profiles/: bench line, the same bench under rocprofv3 --kernel-trace --stats, PMC passes
# (FETCH_SIZE / WRITE_SIZE / TCC hit+miss, one counter set per pass), CG kernel stats, the other formats' bench lines.
# usage (on a machine with an MI355X): bash tools/profile_session.sh [OUT] ; results under OUT (default build/prof, git-ignored)
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-build/prof}
mkdir -p "$OUT"
python bench.py --full > $OUT/bench_n1.json 2> $OUT/bench_n1.err || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -o bench -- python3 bench.py --full --steps 200 --warmup 5 --no-cpu-baseline > $OUT/bench_under_rocprof.json 2> $OUT/rocprof.err || exit 2
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc -o fetch -- python3 tools/pmc_probe.py > $OUT/probe.json 2> $OUT/pmc1.err || exit 3
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc -o write -- python3 tools/pmc_probe.py > $OUT/probe2.json 2> $OUT/pmc2.err || exit 4
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --kernel-trace --output-format csv -d $OUT/pmc -o tcc -- python3 tools/pmc_probe.py > $OUT/probe3.json 2> $OUT/pmc3.err || exit 5
python tools/pmc_summary.py $OUT/pmc $OUT/probe.json $OUT/pmc.json || exit 6
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/cgstats -o cg -- tools/bin/cg_bench --iterations=100 > $OUT/cg_bench.txt 2> $OUT/cg.err || exit 8
for f in ell dia coo hyb; do python bench.py --full --format $f --no-cpu-baseline > $OUT/bench_n1_$f.json 2>/dev/null || exit 7; done
ls $OUT $OUT/stats/* | head -30
