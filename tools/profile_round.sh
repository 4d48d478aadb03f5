#!/bin/bash
# Round profile recipe (run on the GPU box): bench line, rocprofv3 kernel stats, PMC HBM traffic, all written under $OUT.
# A snapshot without .git: pass the commit the library was built from, e.g.  GIT_COMMIT=<short sha> OUT=<dir> tools/profile_round.sh
export GIT_COMMIT=${GIT_COMMIT:-unknown}
R=${GRAFT_REPO_ROOT:-$PWD}
OUT=${OUT:-$R/bench_out}
export TMPDIR=/tmp
mkdir -p $OUT
cd /tmp
python $R/bench.py --full --breakdown $OUT/breakdown.json > $OUT/bench.json 2> $OUT/bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python $R/bench.py --steps 10 --warmup 3 > $OUT/prof.log 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_rd -- python $R/bench.py --steps 3 --warmup 2 > $OUT/pmc_rd.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_wr -- python $R/bench.py --steps 3 --warmup 2 > $OUT/pmc_wr.log 2>&1
python $R/tools/pmc_traffic.py $OUT/pmc_rd $OUT/pmc_wr $OUT/pmc_traffic.json "python bench.py --steps 3 --warmup 2"
# the auxiliary legs (ET configs[3] in both storage modes, 10k-atom water box, TensorNet2): kernel stats + the same two PMC passes
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_aux -- python $R/bench.py --full --aux-only --steps 3 --warmup 2 > $OUT/prof_aux.log 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_rd_aux -- python $R/bench.py --full --aux-only --steps 1 --warmup 1 > $OUT/pmc_rd_aux.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_wr_aux -- python $R/bench.py --full --aux-only --steps 1 --warmup 1 > $OUT/pmc_wr_aux.log 2>&1
python $R/tools/pmc_traffic.py $OUT/pmc_rd_aux $OUT/pmc_wr_aux $OUT/pmc_traffic_aux.json "python bench.py --full --aux-only --steps 1 --warmup 1"
find $OUT/pmc_rd_aux $OUT/pmc_wr_aux -name '*.csv' -size +4M -delete
find $OUT/prof_aux -name '*kernel_trace.csv' -size +8M -delete
# one rank's step of the halo exchange (98k-atom box, 8 slabs: bench.py --full leg one_system_8_slabs): kernel stats + the two PMC passes
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_halo -- python $R/tools/halo_profile.py > $OUT/prof_halo.log 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_rd_halo -- python $R/tools/halo_profile.py > $OUT/pmc_rd_halo.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_wr_halo -- python $R/tools/halo_profile.py > $OUT/pmc_wr_halo.log 2>&1
python $R/tools/pmc_traffic.py $OUT/pmc_rd_halo $OUT/pmc_wr_halo $OUT/pmc_traffic_halo.json "python tools/halo_profile.py"
find $OUT/pmc_rd_halo $OUT/pmc_wr_halo -name '*.csv' -size +4M -delete
# issue-side counters of the dominant kernels (the request ceiling bench.py --full prints next to the HBM one): six --pmc passes
python $R/tools/pmc_issue.py $OUT/pmc_issue.json > $OUT/pmc_issue.log 2>&1
# keep only the summaries (counter CSVs of every dispatch are large)
find $OUT/pmc_rd $OUT/pmc_wr -name '*.csv' -size +4M -delete
find $OUT/prof -name '*kernel_trace.csv' -size +8M -delete
cat $OUT/bench.json
