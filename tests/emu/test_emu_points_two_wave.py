"""The point chain's two-waves-per-SIMD form (k_net_points_w8: 8 row tiles = 256 rows per workgroup on one weight ring, Q / K / V head by head) under the
wave-level emulator, at the smallest shapes where its work split can go wrong.  The emulator runs the same schedule -- ring calls, barriers, feed order,
order of the products per accumulator -- on the host, so a wrong key-tile index, a barrier one wave skips or a misplaced chunk of the head-interleaved
stream shows here.  Tolerances: those of the networks' own parity checks (1e-4 + 1e-4 |ref| + the reference's own jitter sensitivity)."""
import pytest

import parity
import points_split

pytestmark = pytest.mark.emu


def test_one_tile_per_ray_fills_and_overfills_a_workgroup(emu):
  """S = 32: one row tile per ray.  R = 1 leaves seven waves of the workgroup without a ray; 9 rays are 8 + 1 tiles.
  `harsh_many` (48 rays available) has points with at most one valid view: the query mask and the sigma = -1e9 path."""
  parity.check_static_net(emu, 'small', S=32, R=1)
  parity.check_dynamic_net(emu, 'small', S=32, R=1, shift=5.0)
  parity.check_static_net(emu, 'harsh_many', S=32, R=9)
  parity.check_dynamic_net(emu, 'harsh_many', S=32, R=9, shift=5.0)


@pytest.mark.parametrize('name', ['small', 'harsh'])
@pytest.mark.parametrize('S', [64, 128, 40, 100])
def test_two_and_four_tiles_per_ray_with_a_ragged_last_tile(emu, name, S, R=1):
  """Tiles per ray 2 (S = 64, and 40 with a ragged second tile) and 4 (S = 128, and 100 with a ragged fourth), one ray of `small` and of `harsh` (points
  with at most one valid view: the query mask over 2 and 4 key tiles): the attention reads the key tiles of the ray's own waves only, and keys beyond S
  are masked.  (S = 32, one tile per ray, is the test above.)"""
  parity.check_static_net(emu, name, S=S, R=R)
  parity.check_dynamic_net(emu, name, S=S, R=R, shift=5.0)


def test_rays_do_not_depend_on_their_wave(emu):
  """5 rays x 64 samples (two tiles per ray: `wave0 + kt` indexes the shared K image and V table) in one call, and in two calls: the second call's rays sit
  in other waves and workgroups.  Bit for bit (how the rays are cut, and why the static
  network is not cut into a call of three rays: points_split.check_position_independence).  Seven network calls under the emulator: 75 s on a
  loaded 16-core host, the slowest test of this file; the others take 7-27 s each."""
  points_split.check_position_independence(emu, S=64, R=5)
