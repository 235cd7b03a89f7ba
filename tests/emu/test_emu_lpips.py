"""The LPIPS kernels (csrc/dyn_lpips.h) under the wave-level emulator: the same checks as tests/test_gpu_lpips.py through lpips_cases, at the two
smallest shapes and without the entry-point forms (a frame takes seconds here).  Debugging aid in a container without a GPU; -m gpu is
authoritative.  The accuracy pool is that of these two shapes."""
import pytest

import lpips_cases as lc
import lpips_restatement as lr

pytestmark = pytest.mark.emu
SHAPES = ((31, 31), (32, 45))


def test_preparation_bit_exact(emu):
  lc.check_preparation(emu, 32, 45, 'border')


@pytest.mark.parametrize('H,W,kind,seed', [(31, 31, 'noisy', 0), (32, 45, 'close', 1), (31, 31, 'border', 1)])
def test_accuracy_against_float64(emu, H, W, kind, seed):
  lc.check_accuracy(emu, H, W, kind, seed, SHAPES)


def test_masks(emu):
  lc.check_masks(emu, 32, 45, 'border')


def test_identical_images_give_exactly_zero(emu):
  lc.check_identical(emu, 32, 45)


def test_a_masks_sums_do_not_depend_on_its_neighbours(emu):
  lc.check_independence(emu, 31, 31)


def test_value_errors(emu):
  lc.check_value_errors(emu)
