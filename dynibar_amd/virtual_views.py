"""Virtual source views of the monocular path, on the gfx950 kernels: the counterpart of the reference's render_source_vv.py.

ibrnet/data_loaders/monocular.py:312-325, 374-387 load ``dense/source_virtual_views_WxH/NNNNN/KK.png`` and ``dense/source_vv_poses.npy``;
this module writes them.

  python -m dynibar_amd.virtual_views --data_dir DATA --cvd_dir CVD

  * ``render_forward_splat``  -- render_source_vv.py:15-66: one ``dyn_forward_splat`` call (k_splat_project, k_splat_keys, the radix
                                 sort, k_splat_resolve) for a batch of B views;
  * ``render_wander_path``    -- :68-115, pure numpy in float64 like the reference;
  * ``virtual_view_poses``    -- the pose selection and the two axis switches of :195-251;
  * ``sobel_fg_alpha``        -- :118-128 (k_sobel_alpha);
  * ``render_frame_virtual_views`` -- the 8 views of one frame (:253-330) in one batched forward splat and one k_vv_finish;
  * ``relative_transforms``, ``read_record``, ``write_frame_views`` -- the pose algebra, the ``.npz`` decoding and the PNG tree, stated here
                                 once for this module and ``dynibar_amd.ingest``;
  * ``main``                  -- the script: same inputs, same output tree and file names.

Resizing to the working size uses ``torch.nn.functional.interpolate`` (nearest / area / bilinear, ``align_corners=False``) where the
reference uses cv2.resize: that step is NOT cv2-exact.  Everything after it is pinned by the tests (tests/test_gpu_virtual_views.py).
The cv2-style path is ``dynibar_amd.ingest.build_virtual_views`` (``python -m dynibar_amd.ingest --virtual_views``): the float INTER_AREA and
INTER_LINEAR on the device, every frame's views in one batched pass, the same poses and, for the same resized inputs, the same bytes.
"""
from __future__ import annotations

import argparse
import glob
import os

import numpy as np
import torch

from . import splatting as _splatting
from . import _lib
from ._lib import call, params, ptr, stream_of

FINAL_H = 288
NUM_SAMPLES = 4  # virtual views per wander path (render_source_vv.py:214); 2 paths -> 8 views per frame


def _device(*ts):
  for t in ts:
    if isinstance(t, torch.Tensor) and t.is_cuda:
      return t.device
  if not _lib._REQUIRE_DEVICE:  # (tests/emu: the emulator build of the same kernels reads host memory)
    return torch.device('cpu')
  if not torch.cuda.is_available():
    raise RuntimeError('dynibar_amd kernels need a HIP device (cuda:N); none is available (there is no CPU fallback)')
  return torch.device('cuda', torch.cuda.current_device())


def _dev32(t, dev):
  return torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()


def forward_splat(src_imgs, src_depths, r_cam, t_cam, k_src, k_dst, eps=1e-7, mask=False, probes=False):
  """render_forward_splat with everything the kernels produce: dict of feat [B,C,H,W], disp [B,1,H,W], mask [B,1,H,W] (if asked), and
  with ``probes`` the flow [B,2,H,W], importance [B,H,W] and exp(w) [B,H,W] the splat used."""
  _splatting._no_grad_inputs(src_imgs, src_depths, r_cam, t_cam, k_src, k_dst)
  k_src_inv = k_src.inverse()  # formed by torch on k_src's device, as the reference does (:21)
  dev = _device(src_imgs, src_depths, r_cam, t_cam, k_src, k_dst)
  src, depth = _dev32(src_imgs, dev), _dev32(src_depths, dev)
  B, H, W, C = src.shape
  assert depth.shape == (B, H, W), f'src_depths must be [B,H,W] = {(B, H, W)}, got {tuple(depth.shape)}'
  kinv, rot, kdst, t = (_dev32(x, dev).reshape(B, *s) for x, s in ((k_src_inv, (3, 3)), (r_cam, (3, 3)), (k_dst, (3, 3)), (t_cam, (3,))))
  out = {'feat': torch.empty((B, C, H, W), dtype=torch.float32, device=dev), 'disp': torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)}
  if mask:
    out['mask'] = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
  if probes:
    out['flow'] = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
    out['importance'] = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    out['weight_exp'] = torch.empty((B, H, W), dtype=torch.float32, device=dev)
  ws, need = _splatting.workspace(B, H, W, dev)
  p = params('DynForwardSplatParams', B=B, H=H, W=W, C=C, src=ptr(src), depth=ptr(depth), k_src_inv=ptr(kinv), rot=ptr(rot), k_dst=ptr(kdst),
             t=ptr(t), eps=float(eps), feat=ptr(out['feat']), disp=ptr(out['disp']), mask=ptr(out.get('mask')), flow=ptr(out.get('flow')),
             importance=ptr(out.get('importance')), weight_exp=ptr(out.get('weight_exp')), workspace=ptr(ws, torch.uint8), workspace_bytes=need)
  call('dyn_forward_splat', p, stream_of(src))
  return out


def render_forward_splat(src_imgs, src_depths, r_cam, t_cam, k_src, k_dst):
  """render_source_vv.py:15-66.  src_imgs [B,H,W,C], src_depths [B,H,W], r_cam [B,3,3], t_cam [B,3], k_src / k_dst [B,3,3] -- host or
  device tensors; the splat always runs on the GPU.  -> (warp_feature [B,C,H,W], warp_disp [B,1,H,W]) on the device."""
  o = forward_splat(src_imgs, src_depths, r_cam, t_cam, k_src, k_dst)
  return o['feat'], o['disp']


def sobel_fg_alpha(disp, mode='sobel', beta=10.0):
  """render_source_vv.py:118-128: disp [B,1,H,W] -> exp(-beta |sobel(disp)|) [B,1,H,W] (k_sobel_alpha)."""
  if mode != 'sobel':
    raise NotImplementedError(f'sobel_fg_alpha: mode {mode!r} (the reference uses sobel)')
  dev = _device(disp)
  x = _dev32(disp, dev)
  assert x.dim() == 4 and x.shape[1] == 1, f'disp must be [B,1,H,W], got {tuple(x.shape)}'
  B, _, H, W = x.shape
  alpha = torch.empty_like(x)
  call('dyn_sobel_alpha', ptr(x), B, H, W, float(beta), ptr(alpha), stream_of(x))
  return alpha


def vv_finish(feat):
  """render_source_vv.py:313-330: warp_feature [B,C>=4,H,W] -> uint8 [B,H,W,3] (k_vv_finish)."""
  B, C, H, W = feat.shape
  f = feat.float().contiguous()
  out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=f.device)
  call('dyn_vv_finish', ptr(f), B, C, H, W, ptr(out, torch.uint8), stream_of(f))
  return out


def render_wander_path(c2w, hwf, bd_scale, max_disp_=50, xyz=(1, 0, 1)):
  """render_source_vv.py:68-115: 60 poses around c2w [3,4+] whose camera centre moves on an ellipse of radius max_disp_ * bd_scale / focal
  (axes weighted by xyz: cos, sin, cos), rotation unchanged -> (the 60 poses listed twice [120,3,4 + hwf columns], 60).  float64."""
  n = 60
  radius = max_disp_ * bd_scale / hwf[2][0]
  ref = np.asarray(c2w, dtype=np.float64)[:3, :4]
  hwf = np.asarray(hwf, dtype=np.float64)
  out = []
  for i in range(n):
    a = 2.0 * np.pi * float(i) / float(n)
    d = np.array([radius * np.cos(a) * xyz[0], radius * np.sin(a) * xyz[1], radius * np.cos(a) * xyz[2]])
    # c2w . inverse([I | d]) = [R | c - R d]
    out.append(np.concatenate([ref[:, :3], (ref[:, 3] - ref[:, :3] @ d)[:, None], hwf], 1))
  return np.array(out + out), n


def virtual_view_poses(c2w_mats, bounds, hwf):
  """render_source_vv.py:200-251.  c2w_mats [N,4,4] (cam_c2w of every frame), bounds [N] (5th depth percentile of every frame), hwf [3,1]
  -> (vv_poses_final [N,8,3,4] in the switched axes, as saved transposed to source_vv_poses.npy; c2w_mats_vsv [N,8,3,4] switched back)."""
  c2w = np.stack(c2w_mats, 0)[:, :3, :4]
  bd_scale = np.min(np.stack(bounds, 0)) * 0.75
  # the script works in axes (y, x, -z) of the cameras (render_source_vv.py:207-212), in float32, and switches back at :243-251
  poses = np.stack([c2w[..., 1], c2w[..., 0], -c2w[..., 2], c2w[..., 3]], -1).astype(np.float32)
  vv_poses_final = np.zeros((len(poses), NUM_SAMPLES * 2, 3, 4))
  for ii, pose in enumerate(poses):
    for j, (start, disp, xyz) in enumerate(((5, 56 * 1.5, [0., 1., 1.]), (15, 48 * 1.5, [0.5, 1., 0.]))):
      path, n = render_wander_path(pose, hwf, bd_scale, disp, xyz=xyz)
      vv_poses_final[ii, j * NUM_SAMPLES:(j + 1) * NUM_SAMPLES] = path[start:-1:n // NUM_SAMPLES][:NUM_SAMPLES, :3, :4]
  v = vv_poses_final
  c2w_mats_vsv = np.stack([v[..., 1], v[..., 0], -v[..., 2], v[..., 3]], -1)
  return vv_poses_final, c2w_mats_vsv


def relative_transforms(c2w, vv_c2w):
  """``inv([vv_c2w; 0 0 0 1]) @ c2w`` for every frame and view in float64 on the host (render_source_vv.py:297-305): c2w ``[N, 4, 4]``,
  vv_c2w ``[N, V, 3, 4]`` -> (rot float64 ``[N, V, 3, 3]``, t float64 ``[N, V, 3]``)."""
  N, V = len(vv_c2w), len(vv_c2w[0])
  rot, tr = np.empty((N, V, 3, 3)), np.empty((N, V, 3))
  for i in range(N):
    ref = np.asarray(c2w[i], dtype=np.float64)
    for k in range(V):
      tgt = np.eye(4)
      tgt[:3, :4] = vv_c2w[i][k]
      T = np.dot(np.linalg.inv(tgt), ref)
      rot[i, k], tr[i, k] = T[:3, :3], T[:3, 3]
  return rot, tr


def frame_batch(img, disp, K, c2w_ref, vv_c2w):
  """The B = len(vv_c2w) forward-splat inputs of one frame (render_source_vv.py:283-307), on the device: (src [B,H,W,4], depth [B,H,W],
  rot [B,3,3], t [B,3], k [B,3,3]).  img [H,W,3] in [0,1], disp [H,W], K [3,3], c2w_ref [4,4] (float64 poses), vv_c2w [B,3,4]."""
  dev = _device(img, disp)
  img = _dev32(img, dev)
  disp = _dev32(disp, dev)
  H, W = disp.shape
  pred_depth = (1.0 / disp[None, None]) / 10.0
  alpha = sobel_fg_alpha(pred_depth, 'sobel', beta=0.5)[0, 0, ..., None]
  rgba = torch.cat([img * 255.0, alpha], -1)
  B = len(vv_c2w)
  rot, tr = relative_transforms([c2w_ref], [vv_c2w])
  src = rgba[None].expand(B, H, W, 4).contiguous()
  depth = (1.0 / disp)[None].expand(B, H, W).contiguous()
  k = torch.from_numpy(np.array(K)).float()[None].expand(B, 3, 3).contiguous()
  return src, depth, torch.from_numpy(rot[0]).float(), torch.from_numpy(tr[0]).float(), k


def render_frame_virtual_views(img, disp, K, c2w_ref, vv_c2w):
  """All virtual views of one frame (render_source_vv.py:283-330) in one batched forward splat and one finish pass -> uint8 [B,H,W,3]
  on the host (B = 8 for the script's poses)."""
  src, depth, rot, t, k = frame_batch(img, disp, K, c2w_ref, vv_c2w)
  with torch.no_grad():
    o = forward_splat(src, depth, rot, t, k, k)
    return vv_finish(o['feat']).cpu().numpy()


def _resize(a, h, w, mode):
  """[H,W] or [H,W,C] float array -> [h,w(,C)] float32 with F.interpolate (nearest / area / bilinear, align_corners=False).  Not cv2-exact
  (``dynibar_amd.ingest`` has the cv2-style forms on the device: resize_area, resize_linear, resize_nearest)."""
  t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
  x = t[None, None] if t.dim() == 2 else t.permute(2, 0, 1)[None]
  kw = {'align_corners': False} if mode == 'bilinear' else {}
  y = torch.nn.functional.interpolate(x, size=(h, w), mode=mode, **kw)[0]
  return (y[0] if t.dim() == 2 else y.permute(1, 2, 0)).numpy()


def _read_image(path):
  from PIL import Image
  with Image.open(path) as im:
    return np.asarray(im)


def read_record(path):
  """One ``--cvd_dir`` file as the scripts index it -> (img_1 [h, w, 3] channels last, depth [h, w], the stored transposed K [3, 3],
  cam_c2w [4, 4]), in the file's dtypes."""
  with np.load(path) as z:
    return z['img_1'][0].transpose(1, 2, 0), z['depth'][0, 0], z['K'][0, 0, 0], z['cam_c2w'][0]


def _frame_dir(save_dir, i):
  sub = os.path.join(save_dir, '%05d' % i)
  os.makedirs(sub, exist_ok=True)
  return sub


def write_frame_views(save_dir, i, views):
  """The views uint8 [V, H, W, 3] of frame ``i`` -> ``save_dir/NNNNN/KK.png``; returns the paths in view order."""
  from PIL import Image
  sub = _frame_dir(save_dir, i)
  paths = [os.path.join(sub, '%02d.png' % k) for k in range(len(views))]
  for path, view in zip(paths, views):
    Image.fromarray(view).save(path)
  return paths


def main(argv=None):
  """render_source_vv.py:134-330 with the same inputs, output tree and file names."""
  parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  parser.add_argument('--data_dir', type=str, help='data directory')
  parser.add_argument('--cvd_dir', type=str, help='video depth directory')
  args = parser.parse_args(argv)

  data_path = os.path.join(args.data_dir, 'dense')
  pt_out_list = sorted(glob.glob(os.path.join(args.cvd_dir, '*.npz')))
  if not pt_out_list:
    raise FileNotFoundError(f'no *.npz in {args.cvd_dir}')
  png = os.path.join(data_path, 'images', '00000.png')
  o_img = _read_image(png if os.path.exists(png) else os.path.join(data_path, 'images', '00000.jpg'))
  o_ar = float(o_img.shape[1]) / float(o_img.shape[0])
  final_w, final_h = int(round(FINAL_H * o_ar)), int(FINAL_H)
  save_dir = os.path.join(data_path, 'source_virtual_views_%dx%d' % (final_w, final_h))
  os.makedirs(save_dir, exist_ok=True)

  c2w_mats, bounds_mats = [], []
  K = None
  for path in pt_out_list:
    img, pred_depth, Kt, cam_c2w = read_record(path)
    c2w_mats.append(cam_c2w)
    bounds_mats.append(np.percentile(pred_depth, 5))
    K = Kt.transpose()
    K[0, :] *= final_w / img.shape[1]
    K[1, :] *= final_h / img.shape[0]
  h, w, fx, fy = final_h, final_w, K[0, 0], K[1, 1]  # (the last frame's intrinsics, as in the reference)
  hwf = np.array([h, w, (fx + fy) / 2.0]).reshape([3, 1])
  vv_poses_final, c2w_mats_vsv = virtual_view_poses(c2w_mats, bounds_mats, hwf)
  np.save(os.path.join(data_path, 'source_vv_poses.npy'), np.moveaxis(vv_poses_final, 0, -1).astype(np.float32))

  written = []
  for i, path in enumerate(pt_out_list):
    _frame_dir(save_dir, i)  # (before the first device call: an output tree that cannot be written fails here)
    img, pred_depth, Kt, cam_ref2w = read_record(path)
    K = Kt.transpose()
    pred_disp = 1.0 / pred_depth
    K[0, :] *= final_w / img.shape[1]
    K[1, :] *= final_h / img.shape[0]
    assert abs(K[0, 0] - K[1, 1]) / abs(K[0, 0] + K[1, 1]) < 0.005
    img = _resize(img, final_h, final_w, 'area')
    pred_disp = _resize(pred_disp, final_h, final_w, 'bilinear')
    written += write_frame_views(save_dir, i, render_frame_virtual_views(img, pred_disp, K, cam_ref2w, c2w_mats_vsv[i]))
  return written


if __name__ == '__main__':
  main()
