cd $GRAFT_REPO_ROOT
out=${OUT_DIR:-runs}; mkdir -p "$out"          # results folder (OUT_DIR)
python -m pytest tests -q -m gpu -x 2>&1 | tail -4 > $out/t_all_${1:-run}.log
bash tools/profile_bench.sh ${1:-run} > $out/prof_${1:-run}_summary.txt 2>&1
python bench.py --full > $out/bench_${1:-run}.json 2> $out/bench_${1:-run}.err
tail -3 $out/t_all_${1:-run}.log; head -16 $out/prof_${1:-run}_summary.txt; cut -c1-400 $out/bench_${1:-run}.json
