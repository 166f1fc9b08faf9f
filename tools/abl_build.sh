# usage (here, no GPU needed): bash tools/abl_build.sh  -- builds mt_renderer_amd/libmtr_abl<N>.so, N = 1..6: libmtr.so with one part of
# k_geom cut out (MTR_ABL in csrc/k_geom.hip); tools/abl_geom.sh then counts instructions per variant on the GPU box
set -e
cd "$(dirname "$0")/../mt_renderer_amd/csrc"
FL="$(make -s --no-print-directory print-flags)"
OBJS="$(make -s --no-print-directory print-objs)"  # csrc/Makefile owns the flags and the object list
for n in 1 2 3 4 5 6; do
  /opt/rocm/bin/hipcc $FL -DMTR_ABL=$n -c k_geom.hip -o /tmp/k_geom_abl$n.o &
done
wait
for n in 1 2 3 4 5 6; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libmtr_abl$n.so ${OBJS/k_geom.o/\/tmp\/k_geom_abl$n.o} -lz
done
ls -la ../libmtr_abl*.so
