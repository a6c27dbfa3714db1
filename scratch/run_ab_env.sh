# usage: bash scratch/run_ab_env.sh "<bench args>" VAR=a VAR=b ...   -- the bench once per environment setting, back to back
ARGS="$1"; shift
RUN_DIR=${RUN_DIR:-out/ab}
mkdir -p $RUN_DIR
for kv in "$@" "$@"; do
  tag=$(echo $kv | tr '=' '_')
  env $kv timeout -k 10 300 python bench.py $ARGS --full --no-cpu-baseline --no-pipeline > $RUN_DIR/$tag.json 2> $RUN_DIR/$tag.err || { echo "$kv failed"; tail -3 $RUN_DIR/$tag.err; exit 1; }
  python - <<PY
import json
d=json.loads(open("$RUN_DIR/$tag.json").read().strip().splitlines()[-1])
t=d.get("train") or d
print("$kv", "infer", d.get("ms_per_step") if "train" in d else None, "train", t.get("ms_per_step"), t.get("repeat_window_ms_per_step"))
PY
done
