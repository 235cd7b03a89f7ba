"""Scene preparation on the MI355X (dynibar_amd/ingest.py, csrc/dyn_ingest.h) against the numpy restatements of tests/ingest_cases.py (themselves
pinned to independent definitions: tests/test_ingest_cpu.py).  Every comparison is exact: np.array_equal / torch.equal, no tolerance, no
element left out.  The shapes are the smallest at which each branch, edge and work split occurs, plus one production shape per kernel."""
import numpy as np
import pytest
import torch

import ingest_cases as ic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('Hs,Ws,Hd,Wd', ic.AREA_SHAPES)
def test_resize_area(Hs, Ws, Hd, Wd, C):
  """the table branch with both axes partial, the 2 x 2 branch (ties round up), 3 x 2 with the float scale, slivers near the 1e-3 rule, the copy"""
  ic.check_area(DEV, Hs, Ws, Hd, Wd, C)


def test_resize_area_rounds_ties_to_even_in_the_table_branch():
  Hs, Ws, Hd, Wd, C = ic.AREA_TIE_CASE
  ic.check_area(DEV, Hs, Ws, Hd, Wd, C, seed=ic.AREA_TIE_SEED)


def test_resize_area_into_a_pitched_store():
  ic.check_area_pitched(DEV)


def test_resize_area_at_the_frame_size():
  ic.check_area_production(DEV)


def test_refusals():
  ic.check_area_refusals(DEV)
  from dynibar_amd import ingest
  with pytest.raises(ValueError, match='different devices|HIP device'):
    ingest.resize_area(ic.dev_t(ic.u8_image(6, 8, 3), DEV), (4, 3), device='cpu')


@pytest.mark.parametrize('Hs,Ws,Hd,Wd', ic.LINEAR_SHAPES)
def test_resize_linear(Hs, Ws, Hd, Wd):
  ic.check_linear(DEV, Hs, Ws, Hd, Wd)


def test_resize_linear_depth_maps_to_the_frame_size():
  ic.check_linear(DEV, ic.DEPTH_SHAPE[0], ic.DEPTH_SHAPE[1], ic.PRODUCTION[2], ic.PRODUCTION[3], B=2)


def test_resize_nearest():
  ic.check_nearest_cases(DEV)


def test_resize_nearest_at_the_frame_size():
  ic.check_nearest(DEV, ic.raw_mask(ic.PRODUCTION[0], ic.PRODUCTION[1]), (ic.PRODUCTION[3], ic.PRODUCTION[2]))
  ic.check_nearest(DEV, ic.raw_mask(ic.PRODUCTION[0], ic.PRODUCTION[1]), (ic.PRODUCTION[3], ic.PRODUCTION[2]), below=255)


@pytest.mark.parametrize('density', ic.DENSITIES)
@pytest.mark.parametrize('H,W', ic.ERODE_SHAPES)
@pytest.mark.parametrize('r', ic.ERODE_RADII)
def test_erode_disk(H, W, r, density):
  ic.check_erode(DEV, H, W, r, density)


def test_erode_disk_special_masks():
  """all ones stays all ones, a single zero erases exactly the disk, a batch into a pitched store, a width off the tile"""
  ic.check_erode_special(DEV)


@pytest.mark.parametrize('shape,name', [((1, 1), 'uniform'), ((4, 5), 'uniform'), ((4, 5), 'all_equal'), ((33, 31), 'signed_zeros'),
                                        (ic.DEPTH_SHAPE, 'uniform')])
def test_depth_bounds(shape, name):
  ic.check_bounds(DEV, shape, name)


def test_depth_bounds_batch():
  ic.check_bounds(DEV, (9, 13), 'uniform', batch=3)
  ic.check_bounds(DEV, (9, 13), 'signed_zeros', batch=2)


def test_depth_bounds_on_a_zero_have_numpys_value():
  ic.check_bounds_on_a_zero(DEV)


def test_chain_refusals_and_out():
  ic.check_chain_refusals(DEV)


def test_chains():
  ic.check_chains(DEV)


def test_from_decoded():
  ic.check_from_decoded(DEV)


def test_constructors_take_device_tensors():
  ic.check_constructors_take_device_tensors(DEV)


def test_command_line_tool_writes_the_scripts_tree(tmp_path):
  ic.check_cli(DEV, tmp_path)
