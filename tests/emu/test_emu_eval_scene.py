"""The evaluation kernels (k_scene_views_masked, k_eval_mask_pair in csrc/dyn_eval.h) under the wave-level emulator: the checks of
tests/test_gpu_eval_scene.py that need no stream, through eval_scene_cases and the same C ABI, at a few of its shapes.  Debugging aid in a
container without a GPU; -m gpu is authoritative."""
import pytest

import eval_scene_cases as ec

pytestmark = pytest.mark.emu


@pytest.mark.parametrize('H,W', [(5, 7), (17, 19), (16, 16)])
@pytest.mark.parametrize('mask_static', [False, True])
def test_get_all_equals_the_host_sampler(emu, H, W, mask_static):
  for N in (12, 14):
    ec.check_get_all(emu, H, W, N, mask_static)


@pytest.mark.parametrize('H,W', [(5, 7), (17, 19), (16, 16)])
@pytest.mark.parametrize('C', [1, 3])
def test_mask_pair_equals_numpy(emu, H, W, C):
  ec.check_mask_pair(emu, H, W, C)


def test_refusals_never_reach_a_kernel(emu):
  ec.check_entry_refusals(emu)
  ec.check_scene_refusals(ec.device_scene(emu, 5, 7, 14))
