# usage (GPU box): bash tools/sweep_ordered.sh "<flags>" ...   -- ordered-kernel variants on C5 translucent / mixed
set -e
cd $GRAFT_REPO_ROOT/mt_renderer_amd/csrc
FL="$(make -s --no-print-directory print-flags)"
OBJS="$(make -s --no-print-directory print-objs)"  # csrc/Makefile owns the flags and the object list
for v in "$@"; do
  /opt/rocm/bin/hipcc $FL $v -c k_tile.hip -o k_tile.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libmtr.so $OBJS -lz
  echo "== $v"; (cd ../.. && python tools/bench_configs.py translucent 2>&1 | grep "C5" | sed 's/.*4K (1 GPU): //; s/tris_in.*stages_ms/stages_ms/')
done
/opt/rocm/bin/hipcc $FL -c k_tile.hip -o k_tile.o
