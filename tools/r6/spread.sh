#!/bin/bash
# box-to-box / run-to-run spread of the default bench line on the final build (3 runs of the C0 line, no extras)
set -o pipefail
R=$GRAFT_REPO_ROOT
cd $R
O=${OUT_DIR:-$R/bench_out}/r6
mkdir -p $O
for i in 1 2 3; do
  timeout -k 10 300 python -u bench.py --full --no-extras --no-cpu-baseline > $O/spread.json 2> $O/spread.err || { tail -20 $O/spread.err; exit 1; }
  python -c "import json;d=json.loads(open('$O/spread.json').read().strip().splitlines()[-1]);print(d['value'],'Mpix/s',d['ms_per_step'],'ms, k_dcn_sep<0>',d['roofline']['avg_launch_us'],'us, frac',d['roofline']['frac'])"
done
