"""The virtual source views on the MI355X (dynibar_amd/csrc/dyn_splat.h): the splat BITWISE against the sequential float32 restatement
(tests/splat_restatement.py), its determinism across calls and batch sizes, render_forward_splat against float64 and against what the
real reference hands the splat (tests/golden/virtual_views.npz, tests/golden/make_golden_vv.py), the Sobel alpha, the finish step and
the script end to end."""
import os

import numpy as np
import pytest
import torch

import splat_restatement as rs
from dynibar_amd import splatting, virtual_views as vv

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _splat_check(frame, flow, metric=None, modes=splatting.MODES):
  fr, fl = torch.from_numpy(frame).to(DEV), torch.from_numpy(flow).to(DEV)
  for mode in modes:
    m = None if mode in ('summation', 'average') else torch.from_numpy(metric).to(DEV)
    got = splatting.splatting_function(mode, fr, fl, m).cpu().numpy()
    if mode == 'summation':
      want = rs.splat_f32(frame, flow)
    elif mode == 'average':
      want = rs.splat_f32(frame, flow, None, normalize=True)
    else:
      mult = metric[:, 0] if mode == 'linear' else m.exp().cpu().numpy()[:, 0]  # the exp is torch's on the device, as in the package
      want = rs.splat_f32(frame, flow, mult, normalize=True)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=mode)


def test_splat_fractional_flows():
  rng = np.random.RandomState(0)
  B, C, H, W = 3, 5, 37, 61
  _splat_check(rng.uniform(-1, 2, (B, C, H, W)).astype(np.float32), rng.uniform(-6, 6, (B, 2, H, W)).astype(np.float32),
               rng.uniform(-2, 2, (B, 1, H, W)).astype(np.float32))


def test_splat_integer_flows_edge_corners_fall_off():
  rng = np.random.RandomState(1)
  B, C, H, W = 2, 3, 32, 48
  flow = rng.randint(-3, 4, (B, 2, H, W)).astype(np.float32)
  flow[:, 0, :, -1] = 0.0  # the last column: ne / se corners at x = W, off the image
  flow[:, 1, -1, :] = 0.0
  _splat_check(rng.uniform(0, 1, (B, C, H, W)).astype(np.float32), flow, rng.uniform(-2, 2, (B, 1, H, W)).astype(np.float32))


def test_splat_non_finite_and_huge_targets_contribute_nothing():
  rng = np.random.RandomState(2)
  B, C, H, W = 2, 4, 24, 40
  frame = rng.uniform(0, 1, (B, C, H, W)).astype(np.float32)
  flow = rng.uniform(-2, 2, (B, 2, H, W)).astype(np.float32)
  bad = rng.uniform(size=(B, H, W)) < 0.3
  vals = np.array([np.nan, np.inf, -np.inf, 1e10, -1e10, 3e9], np.float32)
  for ch in (0, 1):
    pick = vals[rng.randint(0, len(vals), (B, H, W))]
    flow[:, ch] = np.where(bad, pick, flow[:, ch])
  _splat_check(frame, flow, rng.uniform(-2, 2, (B, 1, H, W)).astype(np.float32))
  only_bad = np.full((1, 2, H, W), np.nan, np.float32)
  only_bad[0, 1] = 1e10
  got = splatting.splatting_function('summation', torch.from_numpy(frame[:1]).to(DEV), torch.from_numpy(only_bad).to(DEV)).cpu().numpy()
  assert (got == 0).all() and not np.signbit(got).any()  # nothing lands: every pixel keeps the sum's +0.0


def test_splat_all_to_one_pile_up():
  rng = np.random.RandomState(3)
  B, C, H, W = 1, 3, 64, 64
  yy, xx = np.mgrid[0:H, 0:W]
  flow = np.stack([20.3 - xx, 41.7 - yy])[None].astype(np.float32)  # every pixel of the image lands at (20.3, 41.7)
  _splat_check(rng.uniform(-1, 1, (B, C, H, W)).astype(np.float32), flow, rng.uniform(-3, 3, (B, 1, H, W)).astype(np.float32))


def _vv_batch(B=8, H=288, W=512, seed=4):
  rng = np.random.RandomState(seed)
  yy, xx = np.mgrid[0:H, 0:W]
  depth = (3.0 + 1.5 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 0.2 * rng.uniform(size=(H, W))).astype(np.float32)
  src = np.concatenate([rng.uniform(0, 255, (H, W, 3)), rng.uniform(0, 1, (H, W, 1))], -1).astype(np.float32)
  f = 0.9 * W
  K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
  ang = np.linspace(0, 2 * np.pi, B, endpoint=False)
  t = np.stack([0.1 * np.cos(ang), 0.08 * np.sin(ang), 0.05 * np.cos(ang)], 1).astype(np.float32)
  rot = np.repeat(np.eye(3, dtype=np.float32)[None], B, 0)
  return (torch.from_numpy(np.repeat(src[None], B, 0)), torch.from_numpy(np.repeat(depth[None], B, 0)), torch.from_numpy(rot),
          torch.from_numpy(t), torch.from_numpy(np.repeat(K[None], B, 0)))


def test_forward_splat_is_deterministic_across_calls_and_batch_sizes():
  src, depth, rot, t, K = (x.to(DEV) for x in _vv_batch())
  a = vv.forward_splat(src, depth, rot, t, K, K, mask=True)
  b = vv.forward_splat(src, depth, rot, t, K, K, mask=True)
  for k in a:
    assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
  for i in range(src.shape[0]):
    one = vv.forward_splat(src[i:i + 1], depth[i:i + 1], rot[i:i + 1], t[i:i + 1], K[i:i + 1], K[i:i + 1], mask=True)
    for k in a:
      assert torch.equal(one[k][0].view(torch.int32), a[k][i].view(torch.int32)), (i, k)


@pytest.mark.parametrize('name', ['a', 'b'])
def test_render_forward_splat_against_float64_and_the_reference(golden_dir, name):
  g = dict(np.load(os.path.join(golden_dir, 'virtual_views.npz')))
  src, depth, R, t, K = (g[f'{name}_{k}'] for k in ('src', 'depth', 'rot', 't', 'k'))
  Kt = torch.from_numpy(K)
  o = vv.forward_splat(torch.from_numpy(src), torch.from_numpy(depth), torch.from_numpy(R), torch.from_numpy(t), Kt, Kt, mask=True,
                       probes=True)
  o = {k: v.cpu().numpy() for k, v in o.items()}
  flow64, imp64, ew64 = rs.project_f64(depth, Kt.inverse().numpy(), R, t, K)
  # points behind the camera land ~1e9 px away through the 1e-8 clamp: there the fp32 pixel is a quotient of cancelling products, compared
  # relatively (the reference's own fp32 values are 1.5e-4 from float64 in scene b); everywhere else within 1e-3 px
  front = np.repeat((np.abs(flow64).max(1) < 1e4)[:, None], 2, 1)
  assert front.mean() > 0.8 and (name == 'a' or (~front).any())
  for ref, rtol in ((flow64, 1e-3), (g[f'{name}_flow'], 1e-5)):
    assert np.abs(o['flow'] - ref)[front].max() < 1e-3
    np.testing.assert_allclose(o['flow'][~front], ref[~front], rtol=rtol)
  np.testing.assert_allclose(o['weight_exp'], ew64, rtol=1e-5)
  np.testing.assert_allclose(o['weight_exp'], np.exp(g[f'{name}_weights'][:, 0].astype(np.float64)), rtol=1e-5)
  np.testing.assert_allclose(o['importance'], g[f'{name}_input_data'][:, 4], rtol=1e-5)
  np.testing.assert_array_equal(o['importance'] > 0, imp64 > 0)
  feat, disp, mask = rs.forward_splat_f32(src, o['flow'], o['importance'], o['weight_exp'])
  for k, want in (('feat', feat), ('disp', disp), ('mask', mask)):
    np.testing.assert_array_equal(_bits(o[k]), _bits(want), err_msg=k)
  f2, d2 = vv.render_forward_splat(torch.from_numpy(src), torch.from_numpy(depth), torch.from_numpy(R), torch.from_numpy(t), Kt, Kt)
  np.testing.assert_array_equal(_bits(f2.cpu().numpy()), _bits(feat))
  np.testing.assert_array_equal(_bits(d2.cpu().numpy()), _bits(disp))


def test_sobel_alpha_and_finish():
  rng = np.random.RandomState(5)
  x = (1.0 / rng.uniform(0.2, 1.0, (2, 1, 64, 96))).astype(np.float32)
  a = vv.sobel_fg_alpha(torch.from_numpy(x).to(DEV), beta=0.5).cpu().numpy()
  np.testing.assert_allclose(a, rs.sobel_alpha_f64(x, 0.5), rtol=2e-5, atol=1e-7)
  feat = rng.uniform(-20, 280, (3, 4, 64, 96)).astype(np.float32)
  feat[:, 3] = rng.uniform(-0.2, 1.2, (3, 64, 96))
  feat[:, 3, :, :2] = 0.8  # mask on along the left edge: the border must not erode it
  got = vv.vv_finish(torch.from_numpy(feat).to(DEV)).cpu().numpy()
  np.testing.assert_array_equal(got, rs.finish_u8(feat))


def _frame(H=288, W=512, seed=6):
  rng = np.random.RandomState(seed)
  yy, xx = np.mgrid[0:H, 0:W]
  img = np.clip(0.5 + 0.4 * np.sin(xx / 17.0)[..., None] * np.cos(yy[..., None] / 11.0 + np.arange(3)), 0, 1).astype(np.float32)
  disp = (0.3 + 0.15 * np.sin(xx / 53.0) * np.cos(yy / 31.0) + 0.2 * (((xx - 200) ** 2 + (yy - 150) ** 2) < 60 ** 2)).astype(np.float32)
  f = 0.9 * W
  K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
  c2w = np.eye(4)
  c2w[:3, 3] = rng.uniform(-0.2, 0.2, 3)
  hwf = np.array([H, W, f]).reshape([3, 1])
  _, vsv = vv.virtual_view_poses([c2w.astype(np.float32)], [1.0 / disp.max()], hwf)
  return img, disp, K, c2w, vsv[0]


def test_render_frame_virtual_views_equals_separate_calls():
  img, disp, K, c2w, vsv = _frame()
  views = vv.render_frame_virtual_views(img, disp, K, c2w, vsv)
  assert views.shape == (8, 288, 512, 3) and views.dtype == np.uint8
  assert 0.3 < (views.max(-1) > 0).mean() < 1.0  # rendered, with holes and an eroded border
  src, depth, rot, t, k = vv.frame_batch(img, disp, K, c2w, vsv)
  for i in range(8):
    feat, _ = vv.render_forward_splat(src[i:i + 1], depth[i:i + 1], rot[i:i + 1], t[i:i + 1], k[i:i + 1], k[i:i + 1])
    np.testing.assert_array_equal(views[i], rs.finish_u8(feat.cpu().numpy())[0])


def test_main_end_to_end(tmp_path):
  from PIL import Image
  H0, W0 = 72, 128  # the clip's own size; the script renders at 288 x 512
  data, cvd = tmp_path / 'scene', tmp_path / 'cvd'
  (data / 'dense' / 'images').mkdir(parents=True)
  cvd.mkdir()
  Image.fromarray(np.zeros((H0 * 4, W0 * 4, 3), np.uint8)).save(data / 'dense' / 'images' / '00000.png')
  rng = np.random.RandomState(7)
  yy, xx = np.mgrid[0:H0, 0:W0]
  for i in range(3):
    K = np.array([[100.0, 0, W0 / 2], [0, 100.0, H0 / 2], [0, 0, 1]], np.float32)
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = [0.05 * i, 0.0, 0.0]
    np.savez(cvd / f'{i:05d}.npz', depth=(2.0 + np.sin(xx / 9.0 + i) * np.cos(yy / 7.0))[None, None].astype(np.float32),
             cam_c2w=c2w[None], img_1=rng.uniform(0, 1, (1, 3, H0, W0)).astype(np.float32), K=K.T[None, None, None])
  written = vv.main(['--data_dir', str(data), '--cvd_dir', str(cvd)])
  poses = np.load(data / 'dense' / 'source_vv_poses.npy')
  assert poses.shape == (8, 3, 4, 3) and poses.dtype == np.float32
  out = data / 'dense' / 'source_virtual_views_512x288'
  assert sorted(os.path.relpath(p, out) for p in written) == [f'{i:05d}/{k:02d}.png' for i in range(3) for k in range(8)]
  for p in written:
    with Image.open(p) as im:
      assert im.size == (512, 288) and im.mode == 'RGB'
