"""The guard of the optimizer step (csrc/dyn_optim.h: k_grad_sumsq, k_grad_stats, k_adam_step_guarded, k_grad_scale) under the wave-level
emulator: the same checks as tests/test_gpu_optim_guard.py through optim_guard_cases, every comparison exact.  Debugging aid in a container
without a GPU; -m gpu is authoritative."""
import pytest

import optim_guard_cases as gc
from dynibar_amd import optim

pytestmark = pytest.mark.emu
SIZES = gc.sizes(optim.CHUNK)


@pytest.mark.parametrize('shape', SIZES)
def test_single_tensor(emu, shape):
  gc.check_single(emu, shape)


@pytest.mark.parametrize('shape', SIZES)
def test_misaligned_views_sum_like_aligned_ones(emu, shape):
  gc.check_misaligned(emu, shape)


def test_600_tensors_from_nan_partials(emu):
  gc.check_many(emu, optim.CHUNK)


@pytest.mark.parametrize('kind', gc.VALUE_CASES)
def test_gradient_values(emu, kind):
  gc.check_values(emu, optim.CHUNK, kind)


@pytest.mark.parametrize('value,mode', gc.NONFINITE_CASES)
def test_injected_nonfinite(emu, value, mode):
  gc.check_nonfinite(emu, optim.CHUNK, value, mode)


def test_ten_guarded_steps_with_steplr_and_torchs_state(emu):
  gc.check_steplr(emu, optim.CHUNK)


def test_grad_norm_and_clip_on_their_own(emu):
  gc.check_standalone(emu, optim.CHUNK)
