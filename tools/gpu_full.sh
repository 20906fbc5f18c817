# GPU-box check: full -m gpu suite, one bench line (gpurun -- bash tools/gpu_full.sh)
set -o pipefail
# logs go to $VTD_OUT (default: vtd_out/)
export O=${VTD_OUT:-vtd_out}
mkdir -p $O
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $O/gpu_tests.log 2>&1 || { tail -30 $O/gpu_tests.log; exit 1; }
tail -2 $O/gpu_tests.log


timeout -k 10 300 python bench.py --full > $O/bench.log 2>&1 || { tail -20 $O/bench.log; exit 1; }
tail -1 $O/bench.log
