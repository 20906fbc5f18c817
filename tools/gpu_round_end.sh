# Round-end evidence on the GPU box: full -m gpu suite (batched parity errors printed),
# headline bench line, rocprofv3 kernel-trace stats of the same bench command (one stream
# and default), PMC FETCH/WRITE passes for `traffic`, per-mode accuracy of the goldens.
#   gpurun --timeout 1200 -- bash tools/gpu_round_end.sh
set -o pipefail
# logs go to $VTD_OUT, a path relative to the repository root (default: vtd_out/)
export O=${VTD_OUT:-vtd_out}
mkdir -p $O
R=$GRAFT_REPO_ROOT
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q -s --timeout 300 --timeout-method thread > $O/gpu_tests.log 2>&1 || { tail -30 $O/gpu_tests.log; exit 1; }
tail -1 $O/gpu_tests.log
timeout -k 10 300 python bench.py --full > $O/bench.log 2>&1 || { tail -20 $O/bench.log; exit 1; }
tail -1 $O/bench.log | cut -c1-300
timeout -k 10 200 python tools/accuracy_report.py --out $O/accuracy.json > $O/accuracy.log 2>&1 || { tail -20 $O/accuracy.log; exit 1; }
cd /tmp && export TMPDIR=/tmp
# kernel evidence on one stream (--streams 1: every launch alone, as in bench.py's profiled
# pass that the roofline object comes from); then the default two-stream command
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $R/$O/prof -o p --output-format csv -- python3 $R/bench.py --steps 10 --warmup 3 --no-cpu-baseline --streams 1 > $R/$O/prof.log 2>&1 || { tail -20 $R/$O/prof.log; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $R/$O/prof2 -o p --output-format csv -- python3 $R/bench.py --steps 10 --warmup 3 --no-cpu-baseline > $R/$O/prof2.log 2>&1 || { tail -20 $R/$O/prof2.log; exit 1; }
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d $R/$O/pmc_fetch -o p --output-format csv -- python3 $R/bench.py --steps 5 --warmup 2 --no-cpu-baseline --streams 1 > $R/$O/pmc_fetch.log 2>&1 || exit 1
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE -d $R/$O/pmc_write -o p --output-format csv -- python3 $R/bench.py --steps 5 --warmup 2 --no-cpu-baseline --streams 1 > $R/$O/pmc_write.log 2>&1 || exit 1
echo done
