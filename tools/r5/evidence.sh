#!/bin/bash
# Round-5 evidence of the current build: the full default bench line (extras + CPU baseline), then the C0
# profile passes of tools/prof_c0.sh (kernel-trace stats, FETCH_SIZE, WRITE_SIZE, SQ/MFMA), TAG=r05.
set -o pipefail
R=$GRAFT_REPO_ROOT
O=${OUT_DIR:-$R/bench_out}/r5
mkdir -p $O
cd $R
timeout -k 10 900 python -u bench.py --full > $O/bench_full.json 2> $O/bench_full.err || { tail -30 $O/bench_full.err; exit 1; }
tail -1 $O/bench_full.json | cut -c1-400
TAG=r05 timeout -k 10 900 bash tools/prof_c0.sh || exit 1
