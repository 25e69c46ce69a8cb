# Round-end GPU runs (from the repo root): full bench line and B = 64 kernel times into the directory given as $1, then tools/profile_r05.sh (kernel stats + PMC passes).
mkdir -p gpurun_out
O=${1:?usage: tools/final_round_runs.sh OUTPUT_DIR}; mkdir -p "$O"
timeout -k 10 500 python bench.py --full > "$O"/f_bench_default.json 2> "$O"/f_bench_default.err || exit 1
timeout -k 10 100 python bench.py --full --batch 64 --steps 200 --profile-steps 20 --loso 0 --cpu-budget 0 --b64-steps 0 --long-steps 0 > "$O"/f_bench_b64.json 2>&1 || exit 1
rm -rf gpurun_out/prof_r05
bash tools/profile_r05.sh > gpurun_out/prof_r05_run.log 2>&1; tail -4 gpurun_out/prof_r05_run.log | cut -c1-160
