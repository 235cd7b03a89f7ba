"""The float INTER_AREA and the batched virtual views on the MI355X: dyn_resize_area_f32 bitwise against its numpy restatement,
ingest.virtual_views bitwise against the per-frame path (virtual_views.render_frame_virtual_views), ingest.build_virtual_views from decoded
records into a resident scene, and the tool's --virtual_views.  The shared checks are in tests/vv_ingest_cases.py."""
import os

import numpy as np
import pytest
import torch

import ingest_cases as ic
import vv_ingest_cases as vc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FILL_MIN = 0.15  # every view of the end-to-end scene is rendered on at least this share of its pixels (measured at 160 x 96: 0.26 .. 0.43)


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('Hs,Ws,Hd,Wd', vc.AREA_F32_CASES)
def test_resize_area_f32(Hs, Ws, Hd, Wd, C):
  vc.check_area_f32(DEV, Hs, Ws, Hd, Wd, C)


def test_resize_area_f32_into_a_pitched_store():
  vc.check_area_f32_pitched(DEV)


def test_resize_area_f32_refusals():
  vc.check_area_f32_refusals(DEV)


def test_virtual_views_equal_the_per_frame_path():
  vc.check_views_equal_the_per_frame_path(DEV)


def test_virtual_views_with_per_frame_intrinsics_that_differ():
  vc.check_per_frame_intrinsics_that_differ(DEV)


def test_virtual_views_in_more_than_one_sort_group():
  vc.check_more_than_one_sort_group(DEV)


def test_virtual_views_one_frame_one_view():
  vc.check_one_frame_one_view(DEV)


def test_virtual_views_with_points_behind_the_camera():
  vc.check_points_behind_the_camera(DEV)


def test_virtual_views_refusals():
  vc.check_views_refusals(DEV)


# ---- from decoded records to a resident scene --------------------------------------------------------------------------------------------
def _records(N, h=48, w=80, seed=0):
  """img_1 [N,h,w,3], depth [N,h,w] (8..10, about 6 % of the pixels at 1.0: the 5th percentile lands on the near pixels and the far majority
  shifts by 63 / 8 px at most), the stored transposed K and cam_c2w [N,4,4]"""
  rng = np.random.default_rng([seed, 41])
  img = rng.random((N, h, w, 3), dtype=np.float32)
  yy, xx = np.mgrid[0:h, 0:w]
  depth = (9.0 + np.sin(xx / 11.0 + np.arange(N)[:, None, None]) * np.cos(yy / 7.0)).astype(np.float32)
  depth[rng.random((N, h, w)) < 0.06] = 1.0
  K = np.array([[70.0, 0, w / 2], [0, 70.0, h / 2], [0, 0, 1]], np.float32)
  c2w = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
  c2w[:, :3, 3] = rng.uniform(-0.1, 0.1, (N, 3)).astype(np.float32)
  return img, depth, np.ascontiguousarray(K.T), c2w


def _write_records(tmp_path, img, depth, Kt, c2w, frame_size):
  from PIL import Image
  data, cvd = tmp_path / 'scene', tmp_path / 'cvd'
  (data / 'dense' / 'images').mkdir(parents=True)
  cvd.mkdir()
  for i in range(len(img)):
    Image.fromarray(np.zeros((frame_size[1], frame_size[0], 3), np.uint8) + np.uint8(10 * i)).save(data / 'dense' / 'images' / f'{i:05d}.png')
    np.savez(cvd / f'batch{i:04d}_out.npz', depth=depth[i][None, None], cam_c2w=c2w[i][None],
             img_1=np.ascontiguousarray(img[i].transpose(2, 0, 1))[None], K=Kt[None, None, None])
  return data, cvd


def test_build_virtual_views_end_to_end(tmp_path):
  _end_to_end(DEV, tmp_path, 7, (48, 80), (160, 96), (320, 192), (480, 288))


def _end_to_end(DEV, tmp_path, N, net, size, frame_size, tool_size):
  """N records of net = (h, w) rendered at size; frame_size: the decoded frames' (w, h), which gives the old tool its size, tool_size"""
  import types
  from dynibar_amd import camera_format, ingest, sample_ray, virtual_views as vv
  from dynibar_amd.scene import DeviceScene
  img, depth, Kt, c2w = _records(N, net[0], net[1])
  near = [np.percentile(d, 5) for d in depth]
  assert all(b < 2.0 for b in near), near  # the 5th percentile is on the near pixels
  views, poses = ingest.build_virtual_views(img, depth, Kt, c2w, size, batch=3, device=DEV)
  assert views.dtype == torch.uint8 and tuple(views.shape) == (N, 8, size[1], size[0], 3) and views.device == torch.device(DEV)
  assert poses.dtype == np.float32 and poses.shape == (8, 3, 4, N)
  fill = (ic.host(views).max(-1) > 0).reshape(N * 8, -1).mean(1)
  assert fill.min() > FILL_MIN and fill.max() < 0.999, fill

  # the poses: the old tool's file for the same records (it renders at 288 rows, so at its size), and virtual_view_poses at this size
  data, cvd = _write_records(tmp_path, img, depth, Kt, c2w, frame_size)
  written = vv.main(['--data_dir', str(data), '--cvd_dir', str(cvd)])
  assert len(written) == 8 * N
  saved = np.load(data / 'dense' / 'source_vv_poses.npy')
  _, poses288 = ingest.build_virtual_views(img, depth, Kt, c2w, tool_size, batch=4, device=DEV)
  assert saved.dtype == poses288.dtype and saved.tobytes() == poses288.tobytes()
  Ks = ingest.scaled_intrinsics(Kt, size[0], size[1], net[1], net[0])
  hwf = np.array([size[1], size[0], (Ks[0, 0] + Ks[1, 1]) / 2.0]).reshape([3, 1])
  final, vsv = vv.virtual_view_poses(list(c2w), near, hwf)
  assert np.moveaxis(final, 0, -1).astype(np.float32).tobytes() == poses.tobytes()

  # the views: ingest.virtual_views on the separately resized arrays
  small = ingest.resize_area_f32(img, size, device=DEV)
  assert np.array_equal(ic.host(small).view(np.uint32), np.stack([vc.resize_area_f32(x, size) for x in img]).view(np.uint32))
  disp = ingest.resize_linear(torch.from_numpy(1.0 / depth).to(DEV), size)
  again = ingest.virtual_views(small, disp, Ks, c2w, vsv)
  assert torch.equal(views, again)

  # into a resident scene: the store is the tensor build_virtual_views made, and a training batch reads its bytes
  dec = ic.decoded_scene(N=N, Hs=2 * size[1], Ws=2 * size[0], size=size)
  dec['virtual_views'], dec['virtual_poses'] = views, camera_format.batch_parse_vv_poses(np.moveaxis(poses, -1, 0))
  scene = DeviceScene.from_decoded(DEV, batch=3, **dec)
  assert scene._vviews.data_ptr() == views.data_ptr()
  args = types.SimpleNamespace(num_source_views=2, max_range=4, init_decay_epoch=10, num_vv=2, mask_src_view=False)
  plan = scene.plan(0, args, rng=np.random.RandomState(5))
  sample_ray.rng.seed(7)
  batch = scene.sampler(plan).random_sample(64, 'uniform')
  rgbs = batch['src_rgbs'][0]
  ref_virtual = [int(v) for v in plan['ref_virtual']]
  assert len(ref_virtual) == 2 and rgbs.shape[0] >= 3
  want = ic.host(views)[int(plan['idx'])][ref_virtual].astype(np.float32) / np.float32(255.0)  # (numpy's division: correctly rounded)
  assert np.array_equal(ic.host(rgbs[-2:]).view(np.uint32), want.view(np.uint32))


def test_tool_writes_the_virtual_views(tmp_path):
  _tool(DEV, tmp_path, 3, (48, 80), (600, 360), (480, 288))


def _tool(DEV, tmp_path, N, net, frame_size, tool_size):
  """frame_size: the decoded frames' (w, h); tool_size: the size both tools derive from it"""
  from PIL import Image
  from dynibar_amd import ingest, virtual_views as vv
  img, depth, Kt, c2w = _records(N, net[0], net[1], seed=1)
  data, cvd = _write_records(tmp_path, img, depth, Kt, c2w, frame_size)
  sized = '%dx%d' % tool_size
  dense = data / 'dense'

  def tree():
    return sorted(os.path.relpath(os.path.join(d, f), dense) for d, _, fs in os.walk(dense) for f in fs)

  assert ingest.main(['--data_dir', str(data), '--cvd_dir', str(cvd), '--batch', '2']) == 0
  plain = tree()
  assert plain == sorted([f'images/{i:05d}.png' for i in range(N)] + [f'images_{sized}/{i:05d}.png' for i in range(N)]
                         + [f'disp/{i:05d}.npy' for i in range(N)] + ['poses_bounds_cvd.npy'])  # what the tool wrote before it had the flag
  assert ingest.main(['--data_dir', str(data), '--cvd_dir', str(cvd), '--batch', '2', '--virtual_views']) == 0
  out = dense / f'source_virtual_views_{sized}'
  mine = sorted(set(tree()) - set(plain))
  views, poses = ingest.build_virtual_views(img, depth, Kt, c2w, tool_size, batch=2, device=DEV)
  views = ic.host(views)
  for i in range(N):
    for k in range(8):
      with Image.open(out / f'{i:05d}' / f'{k:02d}.png') as im:
        assert im.mode == 'RGB' and np.array_equal(np.asarray(im), views[i, k]), (i, k)
  saved = np.load(dense / 'source_vv_poses.npy')
  assert saved.shape == (8, 3, 4, N) and saved.dtype == np.float32 and saved.tobytes() == poses.tobytes()
  # the names are those the old tool reports and writes
  for p in mine:
    os.remove(dense / p)
  written = vv.main(['--data_dir', str(data), '--cvd_dir', str(cvd)])
  assert sorted(os.path.relpath(p, dense) for p in written) + ['source_vv_poses.npy'] == mine
  assert sorted(set(tree()) - set(plain)) == mine
