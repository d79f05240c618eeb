# everything under profiles/ for a round in one GPU call (run from the repo root on the GPU box): PMC passes, kernel-trace
# statistics, the default / ks / vggsound_swin bench lines (--full).  usage: bash tools/collect_profiles.sh <output dir>
# R = round tag (default 03); the logs and bench lines land in <output dir>/fin, the PMC and kernel-trace results where
# tools/pmc_kernels.sh and tools/rocprof_bench.sh put them -- copy what is to be judged into profiles/ afterwards.
R=${GDL_ROUND:-03}
export GDL_ROUND=$R
FIN=${1:?usage: bash tools/collect_profiles.sh <output dir>}/fin
mkdir -p "$FIN"
bash tools/pmc_kernels.sh > "$FIN/pmc_kernels.log" 2>&1
cp gpurun_out/r${R}_pmc_kernels.json profiles/r${R}_pmc_kernels.json 2>/dev/null
bash tools/rocprof_bench.sh r$R > "$FIN/rocprof.log" 2>&1
python bench.py --full > "$FIN/bench_default.json" 2> "$FIN/bench_default.err"
python bench.py --full --workload ks --no-cpu-baseline --no-comparator > "$FIN/bench_ks.json" 2> "$FIN/bench_ks.err"
python bench.py --full --workload vggsound_swin --no-cpu-baseline > "$FIN/bench_swin.json" 2> "$FIN/bench_swin.err"
