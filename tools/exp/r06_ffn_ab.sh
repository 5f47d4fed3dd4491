# Round 6: edtr_ffn (one launch per feed-forward half at the 64x64 level) against the two-GEMM form, same device, bench legs.
O=${1:?usage: r06_ffn_ab.sh OUTPUT_DIR}
mkdir -p "$O"
for v in 1 0 1 0; do
  echo "== EDTR_FFN=$v det512"; EDTR_FFN=$v python bench.py --full --steps 40 --also none --no-cpu-baseline --no-roofline --parity-steps 0 2>/dev/null | python -c "import json,sys; j=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(j['value'], j['ms_per_step'], j['parity_vs_reference_golden']['rel_err_latent'], j['parity_vs_reference_golden']['rel_err_image_samples'])"
done
for v in 1 0; do
  echo "== EDTR_FFN=$v det512s50"; EDTR_FFN=$v python bench.py --full --workload det512s50 --steps 6 --also none --no-cpu-baseline --no-roofline --parity-steps 0 2>/dev/null | python -c "import json,sys; j=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(j['value'], j['ms_per_step'])"
done
echo "== breakdown with the fused launch"
python bench.py --full --steps 8 --also none --no-cpu-baseline --parity-steps 0 --breakdown 2> $O/bench_ffn_breakdown.txt > $O/bench_ffn.json
grep -n "ff\.\|ffn\|layernorm" $O/bench_ffn_breakdown.txt | head
