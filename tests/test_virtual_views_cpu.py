"""Host-side checks of the virtual-source-view path (dynibar_amd.virtual_views, dynibar_amd.splatting): the pose math against what the
real reference computes (tests/golden/virtual_views.npz), the C-ABI entries without a device, the refusal of host tensors, and the
script's argument handling and output paths up to the first device call."""
import os

import numpy as np
import pytest
import torch

from dynibar_amd import _lib, splatting, virtual_views as vv


@pytest.fixture(scope='module')
def golden(golden_dir):
  return dict(np.load(os.path.join(golden_dir, 'virtual_views.npz')))


def test_wander_path_matches_the_reference(golden):
  for key, disp, xyz in (('wander_0', 56 * 1.5, [0., 1., 1.]), ('wander_1', 48 * 1.5, [0.5, 1., 0.])):
    poses, n = vv.render_wander_path(golden['wander_c2w'], golden['wander_hwf'], float(golden['wander_bd_scale']), disp, xyz=xyz)
    assert n == 60 and poses.shape == golden[key].shape == (120, 3, 5) and poses.dtype == np.float64
    np.testing.assert_allclose(poses, golden[key], rtol=1e-12, atol=1e-12)


def test_virtual_view_poses_match_the_reference(golden):
  final, back = vv.virtual_view_poses(list(golden['vv_c2w']), list(golden['vv_bounds']), golden['wander_hwf'])
  assert final.shape == back.shape == (3, 8, 3, 4)
  np.testing.assert_allclose(final, golden['vv_poses'], rtol=1e-12, atol=1e-12)
  # switched back to the cameras' axes: columns (x, y, z, t) = (switched y, switched x, -switched z, t)
  np.testing.assert_array_equal(back[..., 0], final[..., 1])
  np.testing.assert_array_equal(back[..., 2], -final[..., 2])
  # the first virtual view of each path keeps the frame's rotation
  c = golden['vv_c2w'][0]
  np.testing.assert_allclose(back[0, 0, :, :3], c[:3, :3], atol=1e-6)


def test_new_symbols_are_exported_and_validate_without_a_device():
  lib = _lib.lib()
  for name in ('dyn_splat_workspace_bytes', 'dyn_splat', 'dyn_forward_splat', 'dyn_sobel_alpha', 'dyn_vv_finish'):
    assert hasattr(lib, name)
  names = [lib.dyn_profile_name(i).decode() for i in range(lib.dyn_profile_count())]
  for k in ('k_splat_project', 'k_splat_keys', 'k_splat_sort', 'k_splat_resolve', 'k_sobel_alpha', 'k_vv_finish'):
    assert k in names
  assert lib.dyn_splat(None, None) == -1 and b'dyn_splat: null params' in lib.dyn_last_error()
  assert lib.dyn_forward_splat(None, None) == -1 and b'dyn_forward_splat' in lib.dyn_last_error()
  p = _lib.params('DynSplatParams', B=1, C=3, H=0, W=4)
  assert lib.dyn_splat(p, None) == -1 and b'bad shape' in lib.dyn_last_error()
  p = _lib.params('DynSplatParams', B=1, C=3, H=4, W=4, frame=1, flow=1, out=1, workspace=1, workspace_bytes=16)
  assert lib.dyn_splat(p, None) == -1 and b'workspace' in lib.dyn_last_error()
  q = _lib.params('DynForwardSplatParams', B=1, H=4, W=4, C=4, src=1, depth=1, k_src_inv=1, rot=1, k_dst=1, t=1)
  assert lib.dyn_forward_splat(q, None) == -1 and b'feat and disp' in lib.dyn_last_error()
  assert lib.dyn_sobel_alpha(None, 1, 4, 4, 0.5, None, None) == -1 and b'dyn_sobel_alpha' in lib.dyn_last_error()
  assert lib.dyn_vv_finish(1, 1, 3, 4, 4, 1, None) == -1 and b'at least 4 channels' in lib.dyn_last_error()
  with pytest.raises(RuntimeError, match='dyn_splat failed'):
    _lib.call('dyn_splat', None, None)


def test_workspace_size_grows_with_the_shape():
  lib = _lib.lib()
  sizes = [lib.dyn_splat_workspace_bytes(b, h, w) for b, h, w in ((1, 9, 13), (2, 9, 13), (2, 40, 56), (8, 288, 512), (16, 288, 512))]
  assert all(a < b for a, b in zip(sizes, sizes[1:]))
  assert sizes[0] >= 16 * 4 * 9 * 13  # sorted keys and ids, twice
  assert lib.dyn_splat_workspace_bytes(0, 4, 4) == 0 and lib.dyn_splat_workspace_bytes(1, -1, 4) == 0
  assert lib.dyn_splat_workspace_bytes(1 << 10, 1 << 10, 1 << 10) == 0  # beyond the 32-bit contribution ids: unsupported, and said so


def test_splatting_function_refuses_host_tensors_and_checks_arguments():
  frame, flow = torch.zeros(1, 3, 4, 5), torch.zeros(1, 2, 4, 5)
  with pytest.raises(RuntimeError, match='HIP device'):
    splatting.splatting_function('summation', frame, flow)
  with pytest.raises(RuntimeError, match='HIP device'):
    splatting.splatting_function('softmax', frame, flow, torch.zeros(1, 1, 4, 5))
  with pytest.raises(NotImplementedError):
    splatting.splatting_function('max', frame, flow)
  with pytest.raises(AssertionError):
    splatting.splatting_function('summation', frame, flow, torch.zeros(1, 1, 4, 5))
  with pytest.raises(AssertionError):
    splatting.splatting_function('linear', frame, flow, torch.zeros(1, 4, 5))
  with pytest.raises(AssertionError):
    splatting.splatting_function('summation', frame, torch.zeros(1, 2, 4, 6))
  with pytest.raises(RuntimeError, match='forward only'):
    splatting.splatting_function('summation', frame.requires_grad_(True), flow)


def _clip(root, n=2, H0=36, W0=64):
  from PIL import Image
  data, cvd = root / 'scene', root / 'cvd'
  (data / 'dense' / 'images').mkdir(parents=True)
  cvd.mkdir()
  Image.fromarray(np.zeros((H0 * 3, W0 * 3, 3), np.uint8)).save(data / 'dense' / 'images' / '00000.jpg')
  for i in range(n):
    K = np.array([[60.0, 0, W0 / 2], [0, 60.0, H0 / 2], [0, 0, 1]], np.float32)
    np.savez(cvd / f'{i:05d}.npz', depth=np.full((1, 1, H0, W0), 2.0 + i, np.float32), cam_c2w=np.eye(4, dtype=np.float32)[None],
             img_1=np.zeros((1, 3, H0, W0), np.float32), K=K.T[None, None, None])
  return data, cvd


def test_main_writes_poses_and_directories_before_the_first_device_call(tmp_path, monkeypatch):
  data, cvd = _clip(tmp_path)
  seen = []

  class FirstDeviceCall(Exception):
    pass

  def stop(img, disp, K, c2w_ref, vv_c2w):  # the first call that would reach the device
    seen.append((img.shape, disp.shape, np.array(K), vv_c2w.shape))
    raise FirstDeviceCall

  monkeypatch.setattr(vv, 'render_frame_virtual_views', stop)
  with pytest.raises(FirstDeviceCall):
    vv.main(['--data_dir', str(data), '--cvd_dir', str(cvd)])
  poses = np.load(data / 'dense' / 'source_vv_poses.npy')
  assert poses.shape == (8, 3, 4, 2) and poses.dtype == np.float32
  assert (data / 'dense' / 'source_virtual_views_512x288' / '00000').is_dir()  # 288 rows, width from the 00000.jpg aspect ratio
  (img_shape, disp_shape, K, vv_shape), = seen
  assert img_shape == (288, 512, 3) and disp_shape == (288, 512) and vv_shape == (8, 3, 4)
  np.testing.assert_allclose(K[:2, :2], [[480.0, 0], [0, 480.0]])  # focal 60 at 64 x 36, scaled by 8 to 512 x 288


def test_resize_is_interpolate():
  a = np.arange(24, dtype=np.float32).reshape(4, 6)
  np.testing.assert_allclose(vv._resize(a, 2, 3, 'area'), a.reshape(2, 2, 3, 2).mean((1, 3)))
  assert vv._resize(np.zeros((4, 6, 3), np.float32), 8, 12, 'bilinear').shape == (8, 12, 3)
