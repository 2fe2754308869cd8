# usage: r05_tile_ab.sh OUTDIR -- the detect step on 8 tiled clips against 64 distinct ones (--tile-clips), alternating processes
O=${1:?usage: r05_tile_ab.sh OUTDIR}
mkdir -p $O
for t in 8 0 8 0; do
  python bench.py --full --tile-clips $t --no-train --bulk-files 0 --no-cpu-baseline --no-dense-reference --no-split-leg > $O/b_$t.json 2>/dev/null
  python - $O/b_$t.json $t <<'PY'
import json, sys
path, t = sys.argv[1:]
d = json.loads(open(path).read().strip().splitlines()[-1])
print(f"tile {t}:", round(d["value"], 1), round(d["ms_per_step"], 2), "single", round(d["single_lane_graph_replay"]["ms_per_step"], 2), "eager", round(d["eager_with_events"]["ms_per_step"], 2),
      "dets/step", d["config"]["detections_per_step"], "dominant ms/step", round(d["roofline"]["ms_per_step"], 2), "gemm-type", round(d["roofline"]["all_gemm_type_launches_ms_per_step"], 2))
PY
done
