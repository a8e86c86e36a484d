#!/bin/bash
# end-of-round evidence in one bounded call on the GPU box: GPU tests (with the per-op pin reports), the bench line, rocprofv3
# kernel stats of the same command, the PMC traffic passes, one wave-state / matrix-pipe PMC pass for the graded kernel and
# one for the stride-2 slab kernel.   tools/final_run.sh <round> <outdir under gpurun_out>
round=${1:-4}; out=gpurun_out/${2:-final_r$round}
cd "$(dirname "$0")/.."; R=$PWD; export TMPDIR=/tmp
mkdir -p "$out"
(timeout 1500 python -m pytest tests -m gpu -q -rP -rs > "$out/gputest.log" 2>&1; echo "rc=$?" >> "$out/gputest.log") < /dev/null
grep -E "bf16 pin|fp32 taps|\[peaked|SKIPPED|passed|failed|rc=" "$out/gputest.log" | cut -c1-400 > "$out/round${round}_gputest_summary.txt"
tail -n 3 "$out/round${round}_gputest_summary.txt"
# the PMC traffic passes FIRST: bench.py reports roofline.traffic from profiles/round*_pmc_traffic.json only when that reading was
# taken on exactly these sources (hash inside), so the reading has to exist before the bench line is measured
timeout 500 tools/pmc_traffic.sh $round < /dev/null | cut -c1-400
cp gpurun_out/pmc_traffic_r$round/round${round}_pmc_*.{json,csv} profiles/ 2>/dev/null
cp gpurun_out/pmc_traffic_r$round/round${round}_pmc_*.{json,csv} "$out/" 2>/dev/null
timeout 500 python bench.py --full > "$out/bench.json" 2> "$out/bench.err" < /dev/null
python tools/abline.py bench "$out/bench.json" < /dev/null
(cd /tmp && timeout 300 rocprofv3 --kernel-trace --stats -d "$R/$out/stats" -o r$round --output-format csv -- bash -c "cd $R && python bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-clip --no-config1 --no-fp32-w48 --no-two-lanes --no-prepath > $R/$out/bench_under_rocprof.json 2>/dev/null" > /dev/null 2>&1 < /dev/null)
cp "$(find $out/stats -name '*kernel_stats.csv' | head -1)" "$out/round${round}_kernel_stats.csv" 2>/dev/null
head -n 14 "$out/round${round}_kernel_stats.csv" | cut -c1-160
PMC="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT GRBM_GUI_ACTIVE"
(cd /tmp && timeout 300 rocprofv3 --kernel-trace --pmc $PMC -d "$R/$out/pmc_wave" -o w --output-format csv -- bash -c "cd $R && python bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-roofline --no-clip --no-config1 --no-fp32-w48 --no-two-lanes --no-prepath" > /dev/null 2>&1 < /dev/null)
CSV="$(find $out/pmc_wave -name '*counter_collection.csv' | head -1)"
python tools/pmc_mean.py "$CSV" "conv3x3_lds_kernel<48" > "$out/round${round}_pmc_wave.txt" < /dev/null
python tools/pmc_mean.py "$CSV" "conv_s2_slab_kernel" > "$out/round${round}_pmc_s2.txt" < /dev/null
python tools/pmc_mean.py "$CSV" "conv_direct" > "$out/round${round}_pmc_direct.txt" < /dev/null
python tools/pmc_mean.py "$CSV" "stem_fused_kernel" > "$out/round${round}_pmc_stem.txt" < /dev/null
python tools/pmc_mean.py "$CSV" "bottleneck_chain_kernel" > "$out/round${round}_pmc_chain.txt" < /dev/null
cat "$out/round${round}_pmc_wave.txt" "$out/round${round}_pmc_s2.txt"
rm -rf "$out/stats" "$out/pmc_wave"
# the first multi-GPU lease exercises RCCL without a code change: on a box with >= 2 GPUs the two nccl tests of
# tests/test_multi_gpu.py ran above as part of the suite; say here which it was
python - <<'PY' | tee "$out/round${round}_multi_gpu.txt"
import torch
n = torch.cuda.device_count()
print("GPUs on this box: %d -> the 2-rank RCCL tests (bench.py --gpus 2, --clip) %s" % (n, "RAN in the suite above" if n >= 2 else "were SKIPPED (gloo variants ran)"))
PY
# LAST: the driver's smoke() on exactly this tree (it was red because nothing re-ran it after the last change)
(timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > "$out/smoke.log" 2>&1; echo "smoke rc=$?" >> "$out/smoke.log") < /dev/null
tail -n 6 "$out/smoke.log" | cut -c1-300
