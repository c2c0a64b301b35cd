#!/bin/bash
# Round 4: the bench's JSON line for the four one-card configurations (run on the MI355X box through gpurun) -> gpurun_out/r4/lines/, copied to profiles/ afterwards.
set -e
O=gpurun_out/r4/lines; mkdir -p $O
python bench.py --full > $O/r04_bench_line_8b.json 2> $O/8b.err
python bench.py --full --dense > $O/r04_bench_line_dense.json 2> $O/dense.err
python bench.py --full --model qv > $O/r04_bench_line_modelqv.json 2> $O/qv.err
python bench.py --full --bits 8 > $O/r04_bench_line_bits8.json 2> $O/bits8.err
for f in $O/r04_bench_line_*.json; do python -c "
import json,sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(sys.argv[1], round(d['value'],1), round(d['repetitions']['median_ms_per_step'],4), round(d['roofline']['step']['frac'],4), 'traffic' if d['roofline']['traffic'] is not None else 'no-traffic', d.get('parity',{}).get('ok'), d.get('parity',{}).get('ids_checked'))" $f; done
