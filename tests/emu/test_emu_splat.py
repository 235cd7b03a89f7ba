"""The splat, Sobel-alpha and finish kernels of the virtual source views (dynibar_amd/csrc/dyn_splat.h) under the wave-level emulator,
against the restatements of tests/splat_restatement.py: the splat BITWISE, the projection within float64 tolerances.  The authoritative
run is tests/test_gpu_virtual_views.py on the device."""
import numpy as np
import pytest
import torch

import splat_restatement as rs
from dynibar_amd import splatting, virtual_views as vv

pytestmark = pytest.mark.emu

B, C, H, W = 2, 3, 9, 13


def _case(seed, H=H, W=W):
  rng = np.random.RandomState(seed)
  frame = rng.uniform(-2, 3, (B, C, H, W)).astype(np.float32)
  flow = rng.uniform(-3, 3, (B, 2, H, W)).astype(np.float32)
  flow[0, :, 2, :5] = np.round(flow[0, :, 2, :5])  # integer flows: three zero corner weights, edge corners off the image
  flow[1, 0, 4, 3], flow[1, 1, 5, 6], flow[1, 0, 6, 7], flow[1, 1, 7, 8] = np.nan, np.inf, -np.inf, 1e10
  flow[1, :, 0, :4] = [[2.25], [3.5]] - np.array([[0, 1, 2, 3], [0, 0, 0, 0]], np.float32)  # a small pile-up at (2.25, 3.5)
  metric = rng.uniform(-1, 1, (B, 1, H, W)).astype(np.float32)
  return frame, flow, metric


@pytest.mark.parametrize('mode', splatting.MODES)
@pytest.mark.parametrize('hw', [(H, W), (24, 40)])  # one radix pass and one tile; two passes over two tiles
def test_splat_modes_are_bitwise_the_sequential_restatement(emu, mode, hw):
  frame, flow, metric = _case(0, *hw)
  m = None
  if mode in ('linear', 'softmax'):
    m = torch.from_numpy(metric)
  got = splatting.splatting_function(mode, torch.from_numpy(frame), torch.from_numpy(flow), m).numpy()
  if mode == 'summation':
    want = rs.splat_f32(frame, flow)
  elif mode == 'average':
    want = rs.splat_f32(frame, flow, None, normalize=True)
  else:
    mult = metric[:, 0] if mode == 'linear' else torch.from_numpy(metric).exp().numpy()[:, 0]
    want = rs.splat_f32(frame, flow, mult, normalize=True)
  assert got.shape == (B, C) + hw
  np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
  assert np.isfinite(got).all()


def test_forward_splat_probes_and_outputs(emu):
  rng = np.random.RandomState(3)
  src = rng.uniform(0, 255, (B, H, W, 4)).astype(np.float32)
  depth = rng.uniform(1.5, 4.0, (B, H, W)).astype(np.float32)
  f = 0.9 * W
  K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=torch.float32)[None].repeat(B, 1, 1)
  rot = torch.tensor([[[0.999, -0.02, 0.03], [0.02, 0.999, 0.01], [-0.03, -0.01, 0.999]]] * B, dtype=torch.float32)
  t = torch.tensor([[0.1, -0.05, 0.05], [-0.08, 0.1, -0.1]], dtype=torch.float32)
  o = vv.forward_splat(torch.from_numpy(src), torch.from_numpy(depth), rot, t, K, K, mask=True, probes=True)
  o = {k: v.numpy() for k, v in o.items()}
  flow64, imp64, ew64 = rs.project_f64(depth, K.inverse().numpy(), rot.numpy(), t.numpy(), K.numpy())
  assert np.abs(o['flow'] - flow64).max() < 1e-3
  np.testing.assert_allclose(o['importance'], imp64, rtol=1e-5)
  np.testing.assert_allclose(o['weight_exp'], ew64, rtol=1e-5)
  feat, disp, mask = rs.forward_splat_f32(src, o['flow'], o['importance'], o['weight_exp'])
  for k, want in (('feat', feat), ('disp', disp), ('mask', mask)):
    np.testing.assert_array_equal(o[k].view(np.uint32), want.view(np.uint32), err_msg=k)


def test_sobel_alpha_and_finish(emu):
  rng = np.random.RandomState(5)
  x = rng.uniform(0.1, 2.0, (B, 1, H, W)).astype(np.float32)
  a = vv.sobel_fg_alpha(torch.from_numpy(x), beta=0.5).numpy()
  np.testing.assert_allclose(a, rs.sobel_alpha_f64(x, 0.5), rtol=2e-5, atol=1e-7)
  feat = rng.uniform(-20, 280, (B, 4, H, W)).astype(np.float32)
  feat[:, 3] = rng.uniform(-0.2, 1.2, (B, H, W))
  feat[:, 3, 0, :] = 0.9  # mask on along the top edge: the border must not erode it
  got = vv.vv_finish(torch.from_numpy(feat)).numpy()
  np.testing.assert_array_equal(got, rs.finish_u8(feat))
