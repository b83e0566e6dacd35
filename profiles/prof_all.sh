# the round's evidence in one gpurun call:  gpurun -- 'bash profiles/prof_all.sh r02'
#   gpurun_out/<name>/kernel_stats.csv        rocprofv3 --kernel-trace --stats of `bench.py --reads 50000000 --steps 5`
#   gpurun_out/<name>_50M_pmc.json            the counter passes of profiles/prof_pmc.sh, summarised per kernel
#   <lines>/bench_default.json                the default bench run with every leg (--full): stage wall, CPU baseline, rooflines
#                                             (<lines>: the second argument, bench_lines/<name> if none is given)
# then, in the repository:  cp … profiles/ ;  python profiles/make_traffic.py profiles/<name>_50M_pmc.json 50000000
N=${1:-r02}
LINES=${2:-bench_lines/$N}; mkdir -p "$LINES"
bash profiles/prof_stats.sh $N 50000000 > /dev/null
bash profiles/prof_pmc.sh ${N}_pmc 50000000
python3 profiles/summarize_pmc.py gpurun_out/${N}_pmc gpurun_out/${N}_50M_pmc.json > /dev/null
rm -rf gpurun_out/${N}_pmc
python bench.py --full > "$LINES/bench_default.json" 2> "$LINES/bench_default.err"
head -8 gpurun_out/$N/kernel_stats.csv
