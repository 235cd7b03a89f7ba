"""The scene-preparation kernels (csrc/dyn_ingest.h) under the wave-level emulator: the checks of tests/test_gpu_ingest.py through ingest_cases
at the shapes a CPU can afford: no production shape, and no twin of the loader chains, whose erosion always runs at a height of 288.
Debugging aid in a container without a GPU; -m gpu is authoritative."""
import pytest

import ingest_cases as ic

pytestmark = pytest.mark.emu


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('Hs,Ws,Hd,Wd', ic.AREA_SHAPES)
def test_resize_area(emu, Hs, Ws, Hd, Wd, C):
  ic.check_area(emu, Hs, Ws, Hd, Wd, C)


def test_resize_area_into_a_pitched_store(emu):
  ic.check_area_pitched(emu)


def test_resize_area_rounds_ties_to_even_in_the_table_branch(emu):
  Hs, Ws, Hd, Wd, C = ic.AREA_TIE_CASE
  ic.check_area(emu, Hs, Ws, Hd, Wd, C, seed=ic.AREA_TIE_SEED)


@pytest.mark.parametrize('Hs,Ws,Hd,Wd', ic.LINEAR_SHAPES)
def test_resize_linear(emu, Hs, Ws, Hd, Wd):
  ic.check_linear(emu, Hs, Ws, Hd, Wd)


def test_resize_linear_batch(emu):
  ic.check_linear(emu, 9, 13, 4, 5, B=2)


def test_resize_nearest(emu):
  ic.check_nearest_cases(emu)


@pytest.mark.parametrize('H,W', ic.ERODE_EMU_SHAPES)
@pytest.mark.parametrize('r', ic.ERODE_RADII)
def test_erode_disk(emu, H, W, r):
  ic.check_erode(emu, H, W, r, 0.9 if r < 5 else 0.98)


def test_erode_disk_special_masks(emu):
  ic.check_erode_special(emu)


@pytest.mark.parametrize('shape,name', [((1, 1), 'uniform'), ((4, 5), 'uniform'), ((4, 5), 'all_equal'), ((33, 31), 'signed_zeros')])
def test_depth_bounds(emu, shape, name):
  ic.check_bounds(emu, shape, name)


def test_depth_bounds_batch(emu):
  ic.check_bounds(emu, (9, 13), 'uniform', batch=3)


def test_depth_bounds_on_a_zero_have_numpys_value(emu):
  ic.check_bounds_on_a_zero(emu)


def test_refusals(emu):
  ic.check_area_refusals(emu)
