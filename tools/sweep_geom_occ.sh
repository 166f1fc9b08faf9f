# usage (here): bash tools/sweep_geom_occ.sh build   -> mt_renderer_amd/libmtr_gocc<N>.so, N in 4 5 6 7 8 (k_geom's small-draw build with GEOM_OCC_SMALL=N; the other stays at 8)
# usage (GPU box): bash tools/sweep_geom_occ.sh run  -> headline bench (pipelined ms/frame, stage times) and C3 / C5 ms/frame with each
cd "$(dirname "$0")/.."
if [ "$1" = build ]; then
  cd mt_renderer_amd/csrc
  FL="$(make -s --no-print-directory print-flags)"
  OBJS="$(make -s --no-print-directory print-objs)"  # csrc/Makefile owns the flags and the object list
  for n in 4 5 6 7 8; do /opt/rocm/bin/hipcc $FL -DGEOM_OCC=8 -DGEOM_OCC_SMALL=$n -c k_geom.hip -o /tmp/k_geom_occ$n.o & done; wait
  for n in 4 5 6 7 8; do /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libmtr_gocc$n.so ${OBJS/k_geom.o/\/tmp\/k_geom_occ$n.o} -lz; done
  ls ../libmtr_gocc*.so
else
  for n in 4 5 6 7 8; do
    export MTR_LIB_PATH=$PWD/mt_renderer_amd/libmtr_gocc$n.so
    echo "GEOM_OCC_SMALL=$n $(python bench.py --full --steps 500 --warmup 50 --no-cpu-baseline 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], d['roofline']['stage_ms_serial'], d['latency']['ms_per_frame_latency'])")"
    python tools/bench_configs.py "C3" 2>&1 | grep -v amdgpu | cut -c1-60; python tools/bench_configs.py "opaque" 2>&1 | grep -v amdgpu | cut -c1-60
  done
fi
