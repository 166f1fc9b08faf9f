set -e
cd $GRAFT_REPO_ROOT/mt_renderer_amd/csrc
FL="$(make -s --no-print-directory print-flags)"
OBJS="$(make -s --no-print-directory print-objs)"  # csrc/Makefile owns the flags and the object list
mkdir -p ../../bench_out
cp ../../tools/abl/k_tile_vis_abl.hip ./k_tile_vis_abl.hip
for v in "VIS_LANE_MAX=32" "VIS_LANE_MAX=32 -DABL_NO_P2" "VIS_LANE_MAX=64" "VIS_LANE_MAX=256" "VIS_LANE_MAX=256 -DABL_NO_P2"; do
  /opt/rocm/bin/hipcc $FL -D$v -c k_tile_vis_abl.hip -o k_tile_vis.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libmtr.so $OBJS -lz
  cd ../..
  echo "variant=$v" >> bench_out/abl.log
  timeout -k 10 200 python tools/tile_floor.py 2>/dev/null | grep "C2 mesh50k {" >> bench_out/abl.log
  timeout -k 10 200 python bench.py --full --steps 100 --warmup 10 --no-cpu-baseline 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('HL', d['ms_per_step'], d['roofline']['stage_ms'])" >> bench_out/abl.log
  cd mt_renderer_amd/csrc
done
rm -f k_tile_vis_abl.hip
