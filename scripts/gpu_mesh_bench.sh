set -o pipefail
O=${1:?usage: gpu_mesh_bench.sh <outdir>}
mkdir -p $O
for B in 1024; do
timeout -k 10 600 python -u bench.py --full --topology mesh1m --batch $B --steps 2 --warmup 1 --no-cpu --iso-reps 1 > $O/s22_mesh_b$B.json 2> $O/s22_mesh_b$B.err || { echo MESH_FAIL; tail -20 $O/s22_mesh_b$B.err; exit 1; }
python3 -c "import json;d=json.load(open('$O/s22_mesh_b$B.json'));print($B, d['value'], d['gteps'], d['ms_per_step'])"
done
