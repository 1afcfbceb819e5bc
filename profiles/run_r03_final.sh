# Evidence of the final round-3 build, one GPU box: full -m gpu suite, smoke, rocprof kernel stats (cfg4, cfg5-small),
# the --full bench line, parity margins of every fixture, PMC passes, other sizes.  run_r03_final.sh <output dir>
OUT=${1:?usage: run_r03_final.sh <output dir>}
mkdir -p "$OUT"
python -m pytest tests -m gpu -q > $OUT/gpu_tests_full.log 2>&1; tail -2 $OUT/gpu_tests_full.log
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
bash profiles/collect_r03.sh r03z_cfg4 && echo cfg4 stats done
bash profiles/collect_r03.sh r03z_cfg5s --size cfg5-small && echo cfg5s stats done
python3 bench.py --full > $OUT/bench_full.json 2> $OUT/bench_full.err; tail -c 300 $OUT/bench_full.json; echo
python3 profiles/parity_margins.py $OUT/parity_margins.json > $OUT/parity_margins.log 2> $OUT/parity_margins.err; tail -1 $OUT/parity_margins.log | cut -c1-200
bash profiles/collect_pmc.sh r03z_pmc && python3 profiles/pmc_to_json.py r03z_pmc $OUT/pmc_k_row_tasks.json
python3 profiles/iteration_host_profile.py cfg2 > $OUT/host_profile_cfg2.txt 2>&1; head -3 $OUT/host_profile_cfg2.txt | tail -1
python3 bench.py --size cfg5 --steps 3 --warmup 1 --no-cpu-baseline > $OUT/cfg5.json 2> $OUT/cfg5.err; tail -c 300 $OUT/cfg5.json; echo
python3 profiles/cond_estimates.py > $OUT/cond_estimates.txt 2> $OUT/cond_estimates.err; head -4 $OUT/cond_estimates.txt
du -sh "$OUT" | tail -1
