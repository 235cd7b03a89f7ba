"""Flow supervision on the MI355X (dynibar_amd/flow_prep.py, csrc/dyn_flowprep.h) against the numpy restatement of tests/flow_prep_cases.py (itself
pinned to independent definitions: tests/test_flow_prep_cpu.py).  Every comparison is exact: every mask byte, every epi float, every motion
byte and every warp_flow / resize_flow float, no tolerance.  The shapes are chosen for where the kernels can go wrong, not for the workload:
less than a wave, offsets without any partner, odd sizes, three tiles along each grid axis with a ragged last one."""
import numpy as np
import pytest
import torch

import flow_prep_cases as fc
from dynibar_amd import flow_prep

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('subpixel', [32, 0])
@pytest.mark.parametrize('N,H,W', fc.SCENE_SHAPES)
def test_supervision_with_cameras(N, H, W, subpixel):
  fc.check_supervision(DEV, N, H, W, subpixel, True)


@pytest.mark.parametrize('N,H,W', fc.SCENE_SHAPES)
def test_consistency_masks_without_cameras(N, H, W):
  """epi and motion null"""
  fc.check_supervision(DEV, N, H, W, 32, False)


def test_motion_without_the_epipolar_maps():
  fc.check_supervision(DEV, 4, 9, 13, 32, True, want_epi=False)
  fc.check_supervision(DEV, 4, 9, 13, 0, False)


def test_nonfinite_flow():
  fc.check_nonfinite(DEV)


def test_prefilled_outputs_come_back_complete_and_runs_repeat():
  """... also on a side stream"""
  fc.check_prefilled_outputs_and_repeat(DEV)


@pytest.mark.parametrize('Hs,Ws,Hd,Wd,B', [(5, 7, 9, 13, None), (33, 31, 9, 13, None), (9, 13, 4, 5, 2), (6, 7, 6, 7, None), (20, 300, 31, 517, 2)])
def test_resize_flow(Hs, Ws, Hd, Wd, B):
  """enlarging, shrinking, a batch, the copy, more than one block along a row"""
  fc.check_resize(DEV, Hs, Ws, Hd, Wd, B)


def test_warp_flow():
  fc.check_warp(DEV)
  fc.check_warp(DEV, 11, 150)


def test_device_scene_takes_the_masks():
  fc.check_scene_takes_the_masks(DEV)


def test_refusals():
  fc.check_refusals(DEV)
  flows = fc.dev_t(fc.scene_flows(2, 5, 7), DEV)
  with pytest.raises(ValueError, match='different devices|HIP device'):
    flow_prep.consistency_masks(flows, device='cpu')
  with pytest.raises(ValueError, match='out must be'):  # a host tensor where a device one is required
    flow_prep.warp_flow(flows[0, 0], flows[0, 0], out=torch.empty((5, 7, 2)))
  with pytest.raises(ValueError, match='out must be'):
    flow_prep.resize_flow(flows[0, 0], (4, 3), out=torch.empty((3, 4, 2)))


def test_host_inputs_are_uploaded():
  N, H, W = 4, 9, 13
  got = flow_prep.supervision(np.array(fc.scene_flows(N, H, W)), device=DEV)['flow_masks']
  assert got.is_cuda and fc.same_bits(fc.host(got), fc.expected(N, H, W, 32, False)[0])


def test_command_line_tool(tmp_path):
  fc.check_cli(DEV, tmp_path)
