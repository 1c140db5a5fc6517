set -o pipefail
OUT=$(realpath -m "${1:?usage: $0 OUTDIR (where the logs and summaries go)}")
mkdir -p "$OUT"
R=$PWD
cd /tmp && export TMPDIR=/tmp
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d /tmp/p_fold -- python3 $R/bench.py --no-msm --no-config5 --no-configs --no-cpu-baseline > $OUT/bench_fold_profiled.json 2> $OUT/bench_fold_profiled.err
python3 $R/tools/rocprof_summary.py /tmp/p_fold fold0_kernel > $OUT/fold_2p24_kernel_summary.txt 2>&1
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d /tmp/p_gkr -- python3 $R/tools/profile_gkr_round.py 22 20 > $OUT/gkr_run.log 2>&1
python3 $R/tools/rocprof_summary.py /tmp/p_gkr fold_round_evals_kernel round_evals_kernel > $OUT/gkr_sumcheck_2p22_kernel_summary.txt 2>&1
python3 $R/tools/rocprof_timeline.py /tmp/p_gkr 11 "round_evals_kernel<zk::Fr381, 2, false>" > $OUT/gkr_sumcheck_2p22_timeline.txt 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/p_sp -- python3 $R/tools/bench_gkr_sparse.py 22 3 random > $OUT/sparse_run.log 2>&1
python3 $R/tools/rocprof_summary.py /tmp/p_sp fold_round_evals_kernel > $OUT/gkr_sparse_config4_kernel_summary.txt 2>&1
python3 $R/tools/rocprof_timeline.py /tmp/p_sp 24 "phase1_tables_kernel<zk::Fr381, true>" > $OUT/gkr_sparse_config4_layer_timeline.txt 2>&1
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d /tmp/p_b24 -- python3 $R/tools/profile_config5_sumcheck.py 24 > $OUT/basic_run.log 2>&1
python3 $R/tools/rocprof_timeline.py /tmp/p_b24 4 "seg_sums_kernel" > $OUT/basic_sumcheck_2p24_trace.txt 2>&1
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d /tmp/p_gd -- python3 $R/tools/profile_gkr_dense.py 8 5 > $OUT/gkr_dense_run.log 2>&1
python3 $R/tools/rocprof_summary.py /tmp/p_gd > $OUT/gkr_reference_shape_depth8_kernel_summary.txt 2>&1
grep -E "depth|verify" $OUT/gkr_dense_run.log >> $OUT/gkr_reference_shape_depth8_kernel_summary.txt
cd $R
timeout -k 10 120 tools/microbench_round.bin 22 100 1536 > $OUT/microbench_round_2p22.jsonl 2>&1
timeout -k 10 120 tools/microbench_round.bin 22 100 1536 3 >> $OUT/microbench_round_2p22.jsonl 2>&1
echo profiles done
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu_full.log 2>&1
tail -n 2 $OUT/pytest_gpu_full.log
timeout -k 10 300 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
tail -c 300 $OUT/bench_default.json
