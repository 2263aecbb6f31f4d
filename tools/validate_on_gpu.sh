cd $GRAFT_REPO_ROOT
rm -f gpurun_out/gpu_parity_report.txt
OUT=${1:?usage: bash tools/validate_on_gpu.sh <directory for the logs and the bench line>}
mkdir -p "$OUT"
timeout 2400 python -m pytest tests -x -q -m gpu > "$OUT/t_all.log" 2>&1
echo "all gpu tests rc=$?" >> "$OUT/t_all.log"
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/smoke.log" 2>&1
timeout 1500 python bench.py --full > "$OUT/b_full2.json" 2> "$OUT/b_full2.err"
echo "full rc=$?" >> "$OUT/b_full2.err"
tail -4 "$OUT/t_all.log"; tail -2 "$OUT/smoke.log"; tail -3 "$OUT/b_full2.err"
