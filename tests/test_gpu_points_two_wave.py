"""The point chain's two-waves-per-SIMD form (k_net_points_w8: 8 row tiles = 256 rows per workgroup on one weight ring, Q / K / V head by head) on the
MI355X, at the smallest shapes where its work split can go wrong.  Tolerances: those of the networks' own parity checks (1e-4 + 1e-4 |ref| + the
reference's own jitter sensitivity), unchanged."""
import pytest
import torch

import parity
import points_split

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'the -m gpu tests need an MI355X'
  from dynibar_amd import _lib
  _lib.lib()  # fails loudly if the gfx950 library is missing
  return 'cuda:0'


@pytest.mark.parametrize('name', ['small', 'harsh'])
@pytest.mark.parametrize('S', [32, 64, 128, 40, 100])
def test_tiles_per_ray(dev, name, S):
  """Tiles per ray 1, 2 and 4, and a ragged last tile (S = 40: 2 tiles, 8 keys in the second; S = 100: 4 tiles, 4 keys in the fourth).  `harsh` has
  points with at most one valid view: the query mask and the sigma = -1e9 path."""
  parity.check_static_net(dev, name, S=S)
  parity.check_dynamic_net(dev, name, S=S, shift=5.0)


@pytest.mark.parametrize('name,S,R', [('small', 64, 1), ('small', 64, 5), ('harsh_many', 32, 9), ('small', 128, 3)])
def test_partly_filled_and_mixed_workgroups(dev, name, S, R):
  """One ray (six or seven waves of the workgroup have none); 5 rays x 2 tiles = 8 + 2; 9 rays x 1 tile = 8 + 1; 3 rays x 4 tiles = 8 + 4."""
  parity.check_static_net(dev, name, S=S, R=R)
  parity.check_dynamic_net(dev, name, S=S, R=R, shift=5.0)


def test_rays_do_not_depend_on_their_wave(dev):
  """5 rays x 64 samples in one call (tiles 0-9: waves 0-7 of workgroup 0, waves 0-1 of workgroup 1), and in two calls (dynamic 2 + 3: tiles 0-3, then
  0-5; static 1 + 4: tiles 0-1, then 0-7).  Every output of both networks bit for bit (why the static network is not cut into a call of three rays:
  points_split.check_position_independence)."""
  points_split.check_position_independence(dev, S=64, R=5)
