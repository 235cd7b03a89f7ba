"""The view-log kernels (csrc/dyn_viewlog.h) under the wave-level emulator: the same checks as tests/test_gpu_view_log.py through view_log_cases,
at its three smallest shapes (and one that fills more than one tile).  The end-to-end check of
log_view renders a frame, which takes the emulator minutes: it passes there (view_log_cases.check_log_view) but is left to the device.  Debugging aid in a container without a GPU; -m gpu is authoritative."""
import pytest

import view_log_cases as vc

pytestmark = pytest.mark.emu
SHAPES = vc.SHAPES[:3]


@pytest.mark.parametrize('H,W', SHAPES + [(33, 31)])
@pytest.mark.parametrize('name', vc.SCALAR_DATA)
def test_ranges_and_colorize(emu, H, W, name):
  vc.check_ranges_and_colorize(emu, H, W, name)


@pytest.mark.parametrize('H,W', SHAPES + [(33, 31)])
@pytest.mark.parametrize('case', vc.FLOW_CASES)
def test_flow_to_image(emu, H, W, case):
  vc.check_flow(emu, H, W, case)


@pytest.mark.parametrize('H,W,n_flows', [(7, 9, 1), (12, 16, 2), (7, 9, 7)])
def test_panels(emu, H, W, n_flows):
  vc.check_panels(emu, H, W, n_flows)


def test_refusals(emu):
  vc.check_refusals(emu)
