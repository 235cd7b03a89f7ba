"""The optimizer kernel (csrc/dyn_optim.h) under the wave-level emulator: the same checks as tests/test_gpu_optim.py through optim_cases, every
comparison exact.  Debugging aid in a container without a GPU; -m gpu is authoritative."""
import pytest

import optim_cases as oc
from dynibar_amd import optim

pytestmark = pytest.mark.emu
SIZES = oc.sizes(optim.CHUNK)


@pytest.mark.parametrize('shape', SIZES)
def test_single_tensor(emu, shape):
  oc.check_single(emu, shape)


@pytest.mark.parametrize('shape', SIZES)
def test_misaligned_views(emu, shape):
  oc.check_misaligned(emu, shape)


def test_600_tensors_in_6_groups(emu):
  oc.check_many(emu, optim.CHUNK)


def test_grad_none_between_two_updated(emu):
  oc.check_grad_none_between(emu, optim.CHUNK)


def test_first_gradient_at_step_4(emu):
  oc.check_late_first_gradient(emu, optim.CHUNK)


def test_lr_zero_group(emu):
  oc.check_lr_zero(emu)


@pytest.mark.parametrize('kind', oc.VALUE_CASES)
def test_gradient_values(emu, kind):
  oc.check_values(emu, optim.CHUNK, kind)


def test_ten_steps_with_steplr(emu):
  oc.check_steplr(emu, optim.CHUNK)


def test_continues_from_torchs_state(emu):
  oc.check_loaded_state(emu, optim.CHUNK)


def test_zero_grads(emu):
  oc.check_zero_grads(emu, optim.CHUNK)


def test_tensor_refusals(emu):
  oc.check_tensor_refusals(emu)
