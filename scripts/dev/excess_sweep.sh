OUT=${PROFILE_OUT:-profile_out}
mkdir -p $OUT
for v in ${VARIANTS:-"" _c1}; do
  ISOCON_LIB=isocon_amd/lib/libisocon_hip$v.so timeout -k 10 200 python bench.py --full --gpus 1 --steps 15 --warmup 4 --no-cpu-baseline > $OUT/bench_sw$v.json 2> $OUT/bench_sw$v.err
  python - "$v" "$OUT" <<'P'
import json,sys
v, out = sys.argv[1], sys.argv[2]
try:
    d=json.load(open("%s/bench_sw%s.json"%(out, v)))
    k=d["roofline"]["step_kernels_ms"]
    print("variant %-8s step %.3f ms  mm %.3f  lists %.3f  filter %.3f  lanes %.3f  seeds %.3f  rejected_by_filter %d aligned %d" % (v or "base", d["ms_per_step"], k["bound matrix (k_qgram_mm)"], k["survivor lists (k_nn_entry_meta, k_nn_survivors)"], k["block filter (k_nn_block_filter)"], k["pair per lane (k_ed_lanes)"], k["seeds (k_qgram_seed_pairs, k_ed_lanes)"], d["roofline"]["pairs_rejected_by_block_filter"], d["roofline"]["pairs_aligned"]))
except Exception as e:
    print("variant", v, "failed:", e, open("%s/bench_sw%s.err"%(out, v)).read()[-300:])
P
done
