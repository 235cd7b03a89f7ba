"""The numpy restatement of the flow-supervision contract (tests/flow_prep_cases.py) against independent definitions, and the host half of
dynibar_amd/flow_prep.py (fundamental_matrices, the binding).  No GPU: the kernels are compared with the restatement, bit for bit, by
tests/test_gpu_flow_prep.py and tests/emu/test_emu_flow_prep.py."""
import numpy as np
import pytest
import torch

import flow_prep_cases as fc
from dynibar_amd import flow_prep

F32 = np.float32
WARP_SHAPES = [(5, 7), (9, 13), (33, 31), (64, 96)]


@pytest.mark.parametrize('H,W', WARP_SHAPES)
def test_exact_coordinate_warp_against_grid_sample(H, W):
  """subpixel = 0 against float64 grid_sample (bilinear, zero padding, align_corners) at the same fp32 coordinate sums promoted to double.
  Bound 8 * 2^-24 * max|img|: four rounded products and three rounded sums of at most max|img| are 7 half-ulps, the rounded weights (1 - a and
  the products of two of them, which sum to one) another 2 at most, 4.5 * 2^-24 in all, and 8 leaves room; it is not tuned to the code."""
  rng = np.random.default_rng([31, H, W])
  img = rng.standard_normal((H, W, 3)).astype(F32)
  flow = (fc.smooth(rng, H, W, 3.0) + rng.uniform(-0.5, 0.5, (H, W, 2))).astype(F32)
  flow[0, 0], flow[H - 1, W - 1] = (-1.5, -0.25), (1.25, 2.5)  # taps on both sides of two borders
  mx, my = fc.warp_coordinates(flow)
  grid = torch.from_numpy(np.stack([2.0 * mx.astype(np.float64) / (W - 1) - 1.0, 2.0 * my.astype(np.float64) / (H - 1) - 1.0], axis=-1))[None]
  ref = torch.nn.functional.grid_sample(torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None], grid, mode='bilinear', padding_mode='zeros',
                                        align_corners=True)[0].permute(1, 2, 0).numpy()
  err = float(np.abs(fc.warp(img, flow, 0).astype(np.float64) - ref).max())
  bound = 8 * 2.0 ** -24 * float(np.abs(img).max())
  print(f'{H} x {W}: max error {err / (2.0 ** -24 * float(np.abs(img).max())):.3f} * 2^-24 * max|img| (bound 8)')
  assert err <= bound


@pytest.mark.parametrize('H,W', WARP_SHAPES[:3])
def test_quantised_warp_equals_exact_warp_on_the_1_32_grid(H, W):
  rng = np.random.default_rng([32, H, W])
  img = rng.standard_normal((H, W, 2)).astype(F32)
  flow = (rng.integers(-4 * 32, 4 * 32 + 1, (H, W, 2)) / 32.0).astype(F32)  # (pixel + k / 32 is exact in float32 at these sizes)
  a, b = fc.warp(img, flow, 32), fc.warp(img, flow, 0)
  assert fc.same_bits(a, b)
  assert np.abs(a).max() > 0


@pytest.mark.parametrize('a,b', [(1, 0), (0, -1), (2, 3), (-3, 1), (-1, -1)])
def test_integer_translation_is_consistent_exactly_where_its_target_is_inside(a, b):
  """fwd = (a, b), bwd = (-a, -b): the mask is 1 exactly where (col + a, row + b) is inside the image; outside w = 0 and e = |f| >= 0.5 |f| + 0.5"""
  N, H, W = 2, 9, 13
  flows = np.zeros((N, 6, H, W, 2), F32)
  flows[:, 0], flows[:, 3] = (a, b), (-a, -b)
  y, x = np.mgrid[0:H, 0:W]
  for subpixel in (32, 0):
    masks, _, _ = fc.supervision(flows, subpixel=subpixel)
    assert np.array_equal(masks[0, 0], ((x + a >= 0) & (x + a < W) & (y + b >= 0) & (y + b < H)).astype(np.uint8))
    assert np.array_equal(masks[1, 3], ((x - a >= 0) & (x - a < W) & (y - b >= 0) & (y - b < H)).astype(np.uint8))
    assert not masks[0, 1:].any() and not masks[1, :3].any() and not masks[1, 4:].any()  # no partner: no mask
    assert 0 < masks[0, 0].sum() < H * W


def test_static_scene_has_no_epipolar_error_and_a_displaced_block_has():
  """Flows of a static scene, computed in double and rounded to float32 with |flow| < 64, give epi <= 1e-5 px: half an ulp of such a flow is
  1.9e-6, the Sampson distance is to first order the distance to the epipolar line, so at most sqrt(2) times that, and a factor of about 3
  covers F's own rounding and the second-order term.  A block displaced by 3 px across its epipolar lines gives epi > 1 there only."""
  H, W = 33, 31
  K, c2w, flows = fc.static_scene_flow(H, W)
  F = flow_prep.fundamental_matrices(K, c2w)
  assert F.dtype == np.float64 and F.shape == (2, 6, 9)
  assert not F[0, 1:].any() and not F[1, :3].any() and not F[1, 4:].any()
  assert abs(np.linalg.norm(F[0, 0]) - 1) < 1e-12 and abs(np.linalg.norm(F[1, 3]) - 1) < 1e-12
  _, epi, _ = fc.supervision(flows, F)
  print(f'static scene: max epi {float(epi.max()):.3e} px (bound 1e-5)')
  assert float(epi[0, 0].max()) <= 1e-5 and float(epi[1, 3].max()) <= 1e-5
  moved = flows.copy()
  Fm = F[0, 0].reshape(3, 3)
  ys, xs = slice(10, 18), slice(7, 19)
  y, x = np.mgrid[0:H, 0:W].astype(np.float64)
  l0, l1 = Fm[0, 0] * x + Fm[0, 1] * y + Fm[0, 2], Fm[1, 0] * x + Fm[1, 1] * y + Fm[1, 2]
  normal = np.stack([l0, l1], axis=-1) / np.sqrt(l0 * l0 + l1 * l1)[:, :, None]
  moved[0, 0, ys, xs] = (moved[0, 0, ys, xs].astype(np.float64) + 3.0 * normal[ys, xs]).astype(F32)
  masks2, epi2, motion2 = fc.supervision(moved, F, min_votes=1)
  inside = np.zeros((H, W), bool)
  inside[ys, xs] = True
  # (the Sampson distance splits the residual between both images: about 3 / sqrt(2) here, never more than the 3 px to the line)
  assert float(epi2[0, 0][inside].min()) > 1.0 and float(epi2[0, 0][inside].max()) <= 3.0
  assert fc.same_bits(epi2[0, 0][~inside], epi[0, 0][~inside]) and fc.same_bits(epi2[1, 3], epi[1, 3])
  assert not motion2[0][~inside].any()  # the vote: only where a consistent flow leaves its epipolar line
  assert np.array_equal(motion2[0][inside], masks2[0, 0][inside])


def test_pure_rotation_has_no_epipolar_constraint():
  N, H, W = 3, 9, 13
  K = np.tile(np.eye(4), (N, 1, 1))
  K[:, 0, 0] = K[:, 1, 1] = 10.0
  K[:, 0, 2], K[:, 1, 2] = 6.0, 4.0
  c2w = np.tile(np.eye(4), (N, 1, 1))
  for i in range(N):
    c2w[i, :3, :3] = fc.rotation(np.array([0.02 * i, -0.05 * i, 0.01]))
  F = flow_prep.fundamental_matrices(K, c2w)
  assert F.shape == (N, 6, 9) and not F.any()
  _, epi, motion = fc.supervision(fc.scene_flows(N, H, W), F)
  assert not epi.any() and not motion.any()
  F2 = flow_prep.fundamental_matrices(K[0, :3, :3], torch.from_numpy(c2w))  # one 3 x 3 matrix for all frames, poses as a tensor
  assert not F2.any()


def test_fundamental_matrices_annihilate_matching_pixels_in_the_projectors_convention():
  """x_j^T F x_i = 0 for the projections pixel ~ K inv(c2w) X of world points, for every pair in range; zeros out of range"""
  N, H, W = 5, 33, 31
  K, c2w = fc.scene_cameras(N, H, W)
  F = flow_prep.fundamental_matrices(K, c2w)
  X = np.concatenate([np.random.default_rng(33).uniform(-1, 1, (50, 2)), np.random.default_rng(34).uniform(3, 6, (50, 1)), np.ones((50, 1))], axis=1)
  pix = []
  for i in range(N):
    q = (X @ np.linalg.inv(c2w[i]).T)[:, :3] @ K[i, :3, :3].T
    pix.append(q / q[:, 2:3])
  rng = fc.in_range(N)
  for i in range(N):
    for j, o in enumerate(fc.OFFSETS):
      if rng[i, j]:
        Fm = F[i, j].reshape(3, 3)
        l = pix[i] @ Fm.T
        d = np.abs(np.sum(pix[i + o] * l, axis=1)) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2)
        assert d.max() < 1e-9, (i, j, d.max())
      else:
        assert not F[i, j].any()


def test_inputs_exercise_both_mask_values():
  for N, H, W in fc.SCENE_SHAPES:
    for subpixel in (32, 0):
      ones = fc.assert_both_mask_values(fc.expected(N, H, W, subpixel, False)[0], N)
      print(f'{(N, H, W)} subpixel {subpixel}: {100 * ones:.0f} % ones')


def test_bench_tool_counts_the_stated_bytes():
  """tools/flowprepbench.py off the GPU: it loads, its traffic model is the 48 B read + 31 B written per pixel of DESIGN.md section 4.20"""
  import importlib.util
  import os
  path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'flowprepbench.py')
  spec = importlib.util.spec_from_file_location('flowprepbench_under_test', path)
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  assert (tool.READ_BYTES, tool.WRITE_BYTES) == (48, 31) and tool.model_bytes(60) == 60 * 288 * 512 * 79
  if not torch.cuda.is_available():
    with pytest.raises(SystemExit, match='no CPU path'):
      tool.run(2, 1, 1)


def test_binding_and_host_refusals():
  from dynibar_amd import _lib
  lib = _lib.lib()
  for name in ('dyn_flow_resize', 'dyn_warp_flow', 'dyn_flow_supervision'):
    assert hasattr(lib, name) and name in _lib._FUNC_SPECS
  names = [lib.dyn_profile_name(i).decode() for i in range(lib.dyn_profile_count())]
  for k in ('k_flow_resize', 'k_warp_flow', 'k_flow_supervision'):
    assert names.count(k) == 1
  assert lib.dyn_flow_supervision(0, 4, 4, None, None, 0.5, 0.5, 32, 1.0, 2, None, None, None, None) == -1 and b'N=0' in lib.dyn_last_error()
  assert lib.dyn_flow_supervision(1, 65536, 32768, None, None, 0.5, 0.5, 32, 1.0, 2, None, None, None, None) == -1 and b'2^31' in lib.dyn_last_error()
  assert lib.dyn_flow_supervision(1, 4, 4, None, None, 0.5, 0.5, 7, 1.0, 2, None, None, None, None) == -1 and b'subpixel=7' in lib.dyn_last_error()
  assert lib.dyn_warp_flow(1, 4, 4, 5, None, None, None, 32, None) == -1 and b'C=5' in lib.dyn_last_error()
  assert lib.dyn_flow_resize(0, 4, 4, 4, 4, None, None, None) == -1 and b'B=0' in lib.dyn_last_error()
  with pytest.raises((ValueError, RuntimeError), match='HIP device'):  # no CPU fallback
    flow_prep.consistency_masks(np.zeros((2, 6, 4, 4, 2), F32), device='cpu')
  with pytest.raises(ValueError):
    flow_prep.fundamental_matrices(np.eye(3), np.zeros((2, 3, 4)))
  with pytest.raises(ValueError):
    flow_prep.fundamental_matrices(np.zeros((3, 3, 3)), np.tile(np.eye(4), (2, 1, 1)))
