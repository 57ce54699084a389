#!/bin/bash
# per-XCD clock readings of the bench's probe on the default line: tools/gpu_clock_xcd.sh [OUTPUT_DIR]
cd "$(dirname "$0")/.."
O=${1:-$(mktemp -d)}; mkdir -p "$O"
python bench.py --full --record "$O/bench_clock.json" 2>/dev/null | tail -1 | cut -c1-400
python - "$O/bench_clock.json" <<'P'
import json, sys
d=json.loads(open(sys.argv[1]).read())
print('headline', round(d['ms_per_step'],3), d['roofline']['frac'], d['clock']['mean'], [(q['xcd'],round(q['ghz'],3)) for q in d['clock']['per_xcd']])
for s in d['secondary']:
    print(s['name'], round(s['ms_per_step'],3), s.get('kernel_ms'), s.get('issue_frac'), s.get('clock_ghz'), s.get('clock_ghz_xcd_min_max'))
P
python -m pytest tests/test_gpu_bench.py -q -m gpu -x 2>&1 | tail -3
