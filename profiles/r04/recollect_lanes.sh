set -o pipefail
bash profiles/r04/collect.sh gpurun_out/pmc9 C3c C3b C4 PP || exit 1
for c in C3c C3b C4 PP; do cp gpurun_out/pmc9/$c/summary.json profiles/r04/${c}_pmc.json && cp gpurun_out/pmc9/$c/kernel_stats.csv profiles/r04/${c}_kernel_stats.csv || exit 1; done
out=${1:?usage: recollect_lanes.sh <outdir of the bench line>}
timeout -k 10 600 python -u bench.py --full > "$out/bench9.json" 2> "$out/bench9.err" || { tail -20 "$out/bench9.err"; exit 1; }
cat "$out/bench9.json"
