"""The scene kernels (csrc/dyn_scene.h) under the wave-level emulator: the checks of tests/test_gpu_scene.py that need no stream, through
scene_cases, at a few of its shapes.  Debugging aid in a container without a GPU; -m gpu is authoritative."""
import pytest

import scene_cases as sc

pytestmark = pytest.mark.emu


@pytest.mark.parametrize('H,W', [(17, 19), (5, 7), (16, 16)])
@pytest.mark.parametrize('mask_channels', [0, 1, 3])
def test_bit_equality_with_the_host_path(emu, H, W, mask_channels):
  for num_vv, n_rand, mode in ((0, 1, 'uniform'), (3, 13, 'center'), (3, H * W, 'uniform')):
    sc.check_bit_equality(emu, H, W, mask_channels, num_vv, n_rand, mode)
  sc.check_get_all(emu, H, W, mask_channels, 3)


def test_repeated_frames_and_view_limits(emu):
  sc.check_repeated_and_many_views(emu)


def test_bad_indices_never_reach_a_kernel(emu):
  sc.check_bad_indices(emu)
