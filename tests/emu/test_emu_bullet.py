"""The bullet-time kernels (k_scene_views with a target camera in csrc/dyn_scene.h, k_frame_pack_u8 in csrc/dyn_bullet.h) under the wave-level
emulator: the checks of tests/test_gpu_bullet.py that need no stream, through bullet_cases, at a few of its shapes.  Debugging aid in a
container without a GPU; -m gpu is authoritative."""
import pytest

import bullet_cases as bc

pytestmark = pytest.mark.emu


@pytest.mark.parametrize('H,W', [(5, 7), (17, 19), (35, 37)])
@pytest.mark.parametrize('mask_channels', [0, 1, 3])
def test_get_all_equals_the_host_samplers(emu, H, W, mask_channels):
  for num_vv, gt_frame in ((0, None), (3, 5)):
    bc.check_get_all(emu, H, W, mask_channels, num_vv, gt_frame)


@pytest.mark.parametrize('H,W', [(5, 7), (17, 19), (35, 37)])
def test_pack_frames_equals_numpy(emu, H, W):
  for K, gt_frame in ((1, None), (3, None), (1, 4), (3, 11)):
    bc.check_pack(emu, H, W, K, gt_frame)


def test_refusals_never_reach_a_kernel(emu):
  bc.check_views_refusals(emu)
  bc.check_pack_refusals(emu)
