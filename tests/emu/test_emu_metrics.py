"""The frame-metrics kernels (csrc/dyn_metrics.h) under the wave-level emulator: the same checks as tests/test_gpu_metrics.py through
metrics_cases, at the shapes a CPU can afford.  Debugging aid in a container without a GPU; -m gpu is authoritative."""
import pytest

import metrics_cases as mc
import metrics_restatement as mr

pytestmark = pytest.mark.emu
SHAPES = [(7, 7), (9, 13), (40, 56)]


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('name', mr.PREDICTIONS)
@pytest.mark.parametrize('R', mc.RANGES)
def test_frame_metrics(emu, H, W, name, R):
  """preparation bit-exact, the S map against the exact form, the sums of six masks and the six numbers of the frame"""
  mc.check_case(emu, H, W, name, R)


@pytest.mark.parametrize('H,W', SHAPES)
def test_float_target_plain_masks_and_valid_as_mask0(emu, H, W):
  mc.check_float_target_and_plain_masks(emu, H, W)


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('R', mc.RANGES)
def test_entry_points_numpy_and_tensors(emu, H, W, R):
  mc.check_entry_points(emu, H, W, R)


def test_a_masks_sums_do_not_depend_on_its_neighbours(emu):
  mc.check_mask_independence(emu, 40, 56)


def test_value_errors(emu):
  mc.check_value_errors(emu)
