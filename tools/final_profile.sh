#!/bin/bash
# round-end measurement on the GPU box:  bash tools/final_profile.sh <tag> [output directory, default profile_out/]
# 1. PMC HBM traffic (two passes)  2. rocprofv3 --kernel-trace --stats of bench.py  3. the bench line itself
T=$1; R=$GRAFT_REPO_ROOT
O=${2:-$R/profile_out}; mkdir -p "$O"
bash $R/tools/pmc_traffic.sh $T || exit 1
# (parse afterwards with: python3 tools/pmc_traffic_parse.py $T 4 ... -- the run has 1 warm-up + 3 steps)
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_$T" -o p -- python3 $R/bench.py --steps 25 --warmup 5 > "$O/prof_$T.log" 2>&1 || exit 1
cd $R
timeout -k 10 400 python3 bench.py --full --steps 20 --warmup 5 > "$O/${T}_bench.json" 2> "$O/${T}_bench.err" || exit 1
find "$O/prof_$T" -name "*kernel_stats.csv" | head -2
