#!/bin/bash
# full GPU suite + bench line (--full) + rocprofv3 kernel statistics of the same command (tag = $1)
tag=${1:-run}
out=${OUT_DIR:-runs}; mkdir -p "$out"          # results folder (OUT_DIR)
python -m pytest tests -m gpu -x -q 2>&1 | tail -4 > $out/${tag}_tests.log
python bench.py --full > $out/${tag}_bench_default.json 2> $out/${tag}_bench_default.err
bash tools/profile_bench.sh $tag > $out/${tag}_prof.log 2>&1
cat $out/${tag}_tests.log; python -c "
import json;d=json.load(open('$out/${tag}_bench_default.json'));print(d['value'],d['ms_per_step'],d['roofline']['frac'],d['roofline']['traffic'])"
head -20 $out/${tag}_prof.log
