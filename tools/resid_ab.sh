set -o pipefail
# logs go to $VTD_OUT (default: vtd_out/)
export O=${VTD_OUT:-vtd_out}
mkdir -p $O
timeout -k 10 400 python -u -m pytest tests/test_gpu_kernels.py tests/test_gpu_mx8.py tests/test_gpu_model.py -x -q --timeout 120 --timeout-method thread > $O/t.log 2>&1 || { tail -30 $O/t.log; exit 1; }
tail -2 $O/t.log
timeout -k 10 200 python -u tools/accuracy_report.py --out $O/acc_bf16res.json > $O/acc1.log 2>&1 || { tail -20 $O/acc1.log; exit 1; }
VTD_RESID_F32=1 timeout -k 10 200 python -u tools/accuracy_report.py --out $O/acc_f32res.json > $O/acc2.log 2>&1 || { tail -20 $O/acc2.log; exit 1; }
cat $O/acc1.log $O/acc2.log
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/b1.log 2>&1 || { tail -20 $O/b1.log; exit 1; }
tail -1 $O/b1.log
VTD_RESID_F32=1 timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/b2.log 2>&1 || { tail -20 $O/b2.log; exit 1; }
tail -1 $O/b2.log
