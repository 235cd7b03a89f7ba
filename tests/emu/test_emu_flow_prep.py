"""The flow-supervision kernels (csrc/dyn_flowprep.h) under the wave-level emulator: the checks of tests/test_gpu_flow_prep.py through
flow_prep_cases, bit for bit against the numpy restatement.  Debugging aid in a container without a GPU; -m gpu is authoritative."""
import pytest

import flow_prep_cases as fc

pytestmark = pytest.mark.emu


@pytest.mark.parametrize('subpixel', [32, 0])
@pytest.mark.parametrize('N,H,W', fc.SCENE_SHAPES)
def test_supervision_with_cameras(emu, N, H, W, subpixel):
  fc.check_supervision(emu, N, H, W, subpixel, True)


@pytest.mark.parametrize('N,H,W', fc.SCENE_SHAPES)
def test_consistency_masks_without_cameras(emu, N, H, W):
  fc.check_supervision(emu, N, H, W, 32, False)


def test_motion_without_the_epipolar_maps(emu):
  fc.check_supervision(emu, 4, 9, 13, 32, True, want_epi=False)
  fc.check_supervision(emu, 4, 9, 13, 0, False)


def test_nonfinite_flow(emu):
  fc.check_nonfinite(emu)


def test_prefilled_outputs_come_back_complete_and_runs_repeat(emu):
  fc.check_prefilled_outputs_and_repeat(emu)


@pytest.mark.parametrize('Hs,Ws,Hd,Wd,B', [(5, 7, 9, 13, None), (33, 31, 9, 13, None), (9, 13, 4, 5, 2), (6, 7, 6, 7, None)])
def test_resize_flow(emu, Hs, Ws, Hd, Wd, B):
  fc.check_resize(emu, Hs, Ws, Hd, Wd, B)


def test_warp_flow(emu):
  fc.check_warp(emu)


def test_device_scene_takes_the_masks(emu):
  fc.check_scene_takes_the_masks(emu)


def test_refusals(emu):
  fc.check_refusals(emu)


def test_command_line_tool(emu, tmp_path):
  fc.check_cli(emu, tmp_path)
