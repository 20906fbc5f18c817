# GPU-box A/B check of a runtime switch: kernel + model parity tests, the logit-error
# report and one bench line per arm.   gpurun -- bash tools/ab_check.sh VAR=value
set -o pipefail
# logs go to $VTD_OUT (default: vtd_out/)
export O=${VTD_OUT:-vtd_out}
mkdir -p $O
AB="$1"
timeout -k 10 400 python -u -m pytest tests/test_gpu_kernels.py tests/test_gpu_mx8.py tests/test_gpu_model.py -x -q --timeout 120 --timeout-method thread > $O/t.log 2>&1 || { tail -30 $O/t.log; exit 1; }
tail -2 $O/t.log
timeout -k 10 200 python -u tools/accuracy_report.py --out $O/acc_a.json > $O/acc_a.log 2>&1 || { tail -20 $O/acc_a.log; exit 1; }
env $AB timeout -k 10 200 python -u tools/accuracy_report.py --out $O/acc_b.json > $O/acc_b.log 2>&1 || { tail -20 $O/acc_b.log; exit 1; }
grep -h bfloat16 $O/acc_a.log $O/acc_b.log
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/b_a.log 2>&1 || { tail -20 $O/b_a.log; exit 1; }
env $AB timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/b_b.log 2>&1 || { tail -20 $O/b_b.log; exit 1; }
python3 - <<'PY'
import json
import os
for arm in "ab":
    d = json.loads(open(os.path.join(os.environ["O"], f"b_{arm}.log")).read().strip().splitlines()[-1])
    print(arm, d["value"], d["ms_per_step"], {k: v["avg_us"] for k, v in d["kernels"].items()})
PY
