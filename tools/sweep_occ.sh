set -e
cd $GRAFT_REPO_ROOT/mt_renderer_amd/csrc
FL="$(make -s --no-print-directory print-flags)"
OBJS="$(make -s --no-print-directory print-objs)"  # csrc/Makefile owns the flags and the object list
mkdir -p ../../bench_out
for v in 5 6 7 8; do
  /opt/rocm/bin/hipcc $FL -DVIS_OCC=$v -c k_tile_vis.hip -o k_tile_vis.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libmtr.so $OBJS -lz
  cd ../..
  echo "VIS_OCC=$v" >> bench_out/sweep4.log
  timeout -k 10 200 python bench.py --full --steps 100 --warmup 10 --no-cpu-baseline 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], d['roofline']['stage_ms'])" >> bench_out/sweep4.log
  cd mt_renderer_amd/csrc
done
