"""-m gpu: the fall-back edges of the tile kernels' paths -- k_tile.hip's fragment lists against its sub-tile loop (a list
that overflows, the pair cap from both sides, a 64-bit-class triangle in the pass, lists carried over several passes), and
k_tile_vis.hip's order lists and one-at-a-time walk beside them -- on scenes built for one path each
(tests/tile_path_scenes.py).  Before a scene is rendered its premise is computed from its integers and asserted
(tests/test_tile_path_premises.py holds the same premises without a device).  Every scene goes through
tests.helpers.render_gpu -- ordered two-pass, ordered single-pass and auto must agree -- and is compared with the oracle bit
for bit.  These scenes all run 8 waves per bin; tests/test_gpu_vis_waves.py holds k_tile_vis.hip at 2, 4 and 8."""
import pytest

from tests import tile_path_scenes as tp
from tests.helpers import assert_same, render_gpu, render_oracle
from tests.test_tile_path_premises import SCENES, check_premise

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(SCENES))
def test_tile_path_scene_matches_the_oracle(gpu_device, name):
    sc = SCENES[name]()
    check_premise(name, sc)
    draws = sc.draws()
    g = render_gpu(gpu_device, sc.w, sc.h, draws)
    assert_same(g, render_oracle(sc.w, sc.h, draws), name)
    if name == "pair_cap":
        # bin (0, 0) took the lists and bin (2, 0) the loop; the fifth layer of bin (2, 0) is hidden, so where the two bins
        # hold the same triangles (off the opaque half-quad: above the diagonal) their pixels are the same
        for y in range(tp.BIN):
            for x in range(y + 1, tp.BIN):
                assert (g[0][y, x] == g[0][y, x + 2 * tp.BIN]).all() and g[1][y, x] == g[1][y, x + 2 * tp.BIN], (x, y)
