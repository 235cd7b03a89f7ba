"""The extended optimizer step (csrc/dyn_optim.h: k_adamx_step, k_adamx_step_guarded, k_adam_advance) under the wave-level emulator: the same
checks as tests/test_gpu_optim_ext.py through optim_ext_cases, the comparisons with the restatement exact.  Debugging aid in a container
without a GPU; -m gpu is authoritative."""
import pytest

import optim_ext_cases as xc

pytestmark = pytest.mark.emu


@pytest.mark.parametrize('guarded,zero_grads,capturable', xc.BITWISE_CASES)
def test_four_groups_in_one_launch_bitwise(emu, guarded, zero_grads, capturable):
  xc.check_bitwise(emu, guarded, zero_grads, capturable)


@pytest.mark.parametrize('shape', xc.SHAPES)
def test_every_option_on_one_tensor(emu, shape):
  xc.check_single_float_path(emu, shape)


@pytest.mark.parametrize('guarded', (False, True))
def test_old_path_unchanged(emu, guarded):
  xc.check_old_path_unchanged(emu, guarded)


def test_exact_skip(emu):
  xc.check_exact_skip(emu)


@pytest.mark.parametrize('name', sorted(xc.OPTION_SETS))
def test_against_torch_and_state_dicts_both_ways(emu, name):
  xc.check_interop(emu, name)


def test_capturable_state(emu):
  xc.check_capturable_state(emu)
