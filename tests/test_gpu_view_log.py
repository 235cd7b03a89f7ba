"""The logged view panels on the MI355X (dynibar_amd/view_log.py, csrc/dyn_viewlog.h) against the numpy restatements of tests/view_log_cases.py
(themselves equal to the real functions' outputs: tests/test_view_log_cpu.py) and, for the cases it holds, the fixture of the real functions.
Every comparison is exact (torch.equal): the percentile ranges, the colour-mapped images, the flow images byte for byte (a differing byte is
reported with its pixel and angle: the two libraries' double atan2 may differ in the last bit; there is no tolerance), the twelve panels."""
import pytest
import torch

import view_log_cases as vc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('H,W', vc.SHAPES)
@pytest.mark.parametrize('name', vc.SCALAR_DATA)
def test_ranges_and_colorize(H, W, name):
  """one image alone and four in one call (one in the magnitude form), both maps; 65, 1023 and 1025 values, one and several float4 rounds"""
  vc.check_ranges_and_colorize(DEV, H, W, name)


def test_ranges_and_colorize_at_the_frame_size():
  vc.check_ranges_and_colorize(DEV, 288, 512, 'heavy_tail')


@pytest.mark.parametrize('H,W', vc.FLOW_SHAPES)
@pytest.mark.parametrize('case', vc.FLOW_CASES)
def test_flow_to_image(H, W, case):
  vc.check_flow(DEV, H, W, case)


@pytest.mark.parametrize('H,W,n_flows', [(12, 16, 2), (12, 16, 7), (35, 37, 2), (35, 37, 7)])
def test_panels(H, W, n_flows):
  vc.check_panels(DEV, H, W, n_flows)


def test_stacks_of_one_six_and_seven_flows():
  vc.check_stacks_of(DEV)


def test_panels_take_three_launches_and_one_copy():
  """the kernels of a panels() call by the library's own per-kernel counters; .cpu() moves the packed buffer once"""
  import numpy as np
  from dynibar_amd import _lib, view_log
  ret, gt_img, gt_disp, gt_flows = vc.synthetic_groups(12, 16, 6)
  dret, dgt = vc.to_device(ret, DEV), (gt_img.to(DEV), gt_disp.to(DEV), gt_flows.to(DEV))
  view_log.panels(dret, *dgt)  # (the tables are uploaded by the first call)
  lib = _lib.lib()
  n = lib.dyn_profile_count()
  ms, cnt = np.zeros(n, np.float32), np.zeros(n, np.int32)
  lib.dyn_profile_enable(1)
  try:
    lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
    got = view_log.panels(dret, *dgt)
    torch.cuda.synchronize()
    lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
  finally:
    lib.dyn_profile_enable(0)
  launched = {lib.dyn_profile_name(i).decode(): int(c) for i, c in enumerate(cnt) if c}
  assert launched == {'k_viewlog_ranges': 1, 'k_viewlog_flow_max': 1, 'k_viewlog_panels': 1}, launched
  import test_gpu_scene as tgs
  with tgs._Copies() as seen:
    host = got.cpu()
  assert len(seen.d2h) == 1 and seen.h2d == [], (seen.d2h, seen.h2d)
  assert host.buffer.is_pinned() and host.buffer.numel() == got.buffer.numel()


def test_log_view_end_to_end():
  vc.check_log_view(DEV)


def test_refusals():
  vc.check_refusals(DEV)
  from dynibar_amd import view_log
  x = torch.zeros((5, 6), dtype=torch.float32)
  with pytest.raises(RuntimeError, match='HIP device'):
    view_log.colorize(x)
  ret, gt_img, gt_disp, gt_flows = vc.synthetic_groups(5, 6, 2)
  with pytest.raises(RuntimeError, match='HIP device'):
    view_log.panels(ret, gt_img, gt_disp, gt_flows)
  dret = vc.to_device(ret, DEV)
  with pytest.raises(ValueError):
    view_log.panels(dret, gt_img.to(DEV)[:4], gt_disp.to(DEV), gt_flows.to(DEV))
  with pytest.raises(ValueError):
    view_log.panels(dret, gt_img.to(DEV).double(), gt_disp.to(DEV), gt_flows.to(DEV))
