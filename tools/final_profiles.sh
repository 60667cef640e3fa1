#!/usr/bin/env bash
# tools/final_profiles.sh NAME OUTDIR -- everything behind profiles/NAME_*: kernel trace + stats, the PMC passes, pmc_latest.json,
# and (second step, because bench.py reads pmc_latest.json) the line of `bench.py --gpus 1 --steps 20 --warmup 5 --full`;
# copies of the four files go to OUTDIR.  Run on an MI355X:
#   bash tools/final_profiles.sh r04_final OUTDIR
NAME="${1:-final}"
OUT="${2:?usage: tools/final_profiles.sh NAME OUTDIR}"
bash tools/prof.sh fin --steps 40 --warmup 5 --repeats 3 --full --no-cpu-baseline --no-extras --views-in-flight 1 > /dev/null 2>&1
bash tools/pmc.sh fin > /dev/null 2>&1
python tools/summarize_profiles.py fin "$NAME" | tail -3
python bench.py --gpus 1 --steps 20 --warmup 5 --full 2>/dev/null | tail -1 > profiles/${NAME}_bench.json
mkdir -p "$OUT"; cp profiles/${NAME}_kernel_stats.txt profiles/${NAME}_pmc.txt profiles/pmc_latest.json profiles/${NAME}_bench.json "$OUT"/
cut -c1-400 profiles/${NAME}_bench.json
