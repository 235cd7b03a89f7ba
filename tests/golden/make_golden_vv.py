"""Golden vectors of the virtual-source-view path, recorded from the REAL reference script (build container only).

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vv.py

Imports render_source_vv.py of the reference read-only, with stub modules for its imports that play no part in what is recorded (cv2,
imageio, kornia, skimage) and a recording stub for the third-party ``splatting.splatting_function``.  With ``torch.Tensor.cuda`` made the
identity for the duration, the reference's own ``render_forward_splat`` runs on the CPU and hands the stub its exact ``input_data``,
``flow`` and ``weights`` -- what the splat receives.  Recorded, for two small scenes (one with points behind the target camera): the
inputs, those three tensors; and ``render_wander_path`` for both parameter sets the script uses.  -> tests/golden/virtual_views.npz
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refimport  # noqa: E402

REC = []


def _stub_modules():
  for name in ('cv2', 'imageio', 'imageio.v2', 'kornia', 'skimage', 'skimage.morphology'):
    sys.modules.setdefault(name, types.ModuleType(name))
  sys.modules['imageio'].v2 = sys.modules['imageio.v2']
  sys.modules['skimage'].morphology = sys.modules['skimage.morphology']
  sp = types.ModuleType('splatting')

  def splatting_function(splatting_type, frame, flow, importance_metric=None, eps=1e-7):
    REC.append({'type': splatting_type, 'input_data': frame.clone(), 'flow': flow.clone(), 'weights': importance_metric.clone()})
    B, C, H, W = frame.shape
    return torch.zeros(B, C - 1, H, W, dtype=frame.dtype)

  sp.splatting_function = splatting_function
  sys.modules['splatting'] = sp


def import_script():
  _stub_modules()
  sys.dont_write_bytecode = True
  spec = importlib.util.spec_from_file_location('render_source_vv', os.path.join(refimport.REF_ROOT, 'render_source_vv.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def rot(ax, ay, az):
  cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
  Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
  Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
  Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
  return Rz @ Ry @ Rx


def scene(seed, H=40, W=56, behind=False):
  """B = 2 RGBA sources with depths spanning more than a factor 2 and small camera motions; `behind`: the second view's camera moves
  forward past the foreground, whose points then lie behind it (new_z < 0, pixel coordinates ~1e8-1e10 through the 1e-8 clamp)."""
  rng = np.random.RandomState(seed)
  B = 2
  src = rng.uniform(0, 255, (B, H, W, 4)).astype(np.float32)
  src[..., 3] = rng.uniform(0, 1, (B, H, W))
  yy, xx = np.mgrid[0:H, 0:W]
  depth = np.empty((B, H, W), np.float32)
  for b in range(B):
    base = 4.5 + 1.5 * np.sin(xx / 9.0 + b) * np.cos(yy / 7.0)  # background 3 .. 6
    fg = ((xx - W * 0.4) ** 2 + (yy - H * 0.5) ** 2) < (min(H, W) * 0.25) ** 2
    depth[b] = np.where(fg, 1.2 + 0.3 * rng.uniform(size=(H, W)), base)
  f = 0.9 * W
  K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]], np.float32)
  Ks = np.stack([K, K * np.array([[1.02], [0.98], [1]], np.float32)])
  R = np.stack([rot(0.02, -0.03, 0.01), rot(-0.01, 0.04, -0.02)]).astype(np.float32)
  t = np.array([[0.15, -0.05, 0.1], [-0.1, 0.08, -0.2]], np.float32)
  if behind:
    t[1] = [0.05, 0.0, -2.0]  # foreground (depth 1.2 .. 1.5) ends up at z < -0.4, background (3 .. 6) in front at z > 0.9
  return src, depth, R, t, Ks


def main():
  ref = import_script()
  out = {}
  orig = torch.Tensor.cuda
  torch.Tensor.cuda = lambda self, *a, **k: self
  try:
    for name, kw in (('a', dict(seed=0)), ('b', dict(seed=1, behind=True))):
      src, depth, R, t, K = scene(**kw)
      REC.clear()
      ref.render_forward_splat(torch.from_numpy(src), torch.from_numpy(depth), torch.from_numpy(R), torch.from_numpy(t), torch.from_numpy(K),
                               torch.from_numpy(K))
      rec, = REC
      assert rec['type'] == 'softmax'
      for k, v in (('src', src), ('depth', depth), ('rot', R), ('t', t), ('k', K)):
        out[f'{name}_{k}'] = v
      for k in ('input_data', 'flow', 'weights'):
        out[f'{name}_{k}'] = rec[k].numpy()
  finally:
    torch.Tensor.cuda = orig
  rng = np.random.RandomState(7)
  c2w = np.concatenate([rot(0.1, -0.2, 0.05), rng.uniform(-1, 1, (3, 1))], 1).astype(np.float32)
  hwf = np.array([288, 512, np.float32(455.3)]).reshape([3, 1])
  out['wander_c2w'], out['wander_hwf'], out['wander_bd_scale'] = c2w, hwf, np.float64(1.37)
  out['wander_0'], n0 = ref.render_wander_path(c2w, hwf, 1.37, 56 * 1.5, xyz=[0., 1., 1.])
  out['wander_1'], n1 = ref.render_wander_path(c2w, hwf, 1.37, 48 * 1.5, xyz=[0.5, 1., 0.])
  assert n0 == n1 == 60
  # the virtual-view poses of a 3-frame clip: frames' cam_c2w, their 5th depth percentiles; each frame's pose in the script's switched
  # axes (columns y, x, -z, t of cam_c2w, in float32), the reference's two wander paths around it and the 4 + 4 poses the script keeps
  c2ws = np.stack([np.concatenate([np.concatenate([rot(*rng.uniform(-0.2, 0.2, 3)), rng.uniform(-1, 1, (3, 1))], 1), [[0, 0, 0, 1]]], 0)
                   for _ in range(3)]).astype(np.float32)
  bounds = rng.uniform(1.0, 3.0, 3)
  out['vv_c2w'], out['vv_bounds'] = c2ws, bounds
  sel = []
  for c in c2ws:
    pose = np.stack([c[:3, 1], c[:3, 0], -c[:3, 2], c[:3, 3]], 1).astype(np.float32)
    p0, _ = ref.render_wander_path(pose, hwf, bounds.min() * 0.75, 56 * 1.5, xyz=[0., 1., 1.])
    p1, _ = ref.render_wander_path(pose, hwf, bounds.min() * 0.75, 48 * 1.5, xyz=[0.5, 1., 0.])
    sel.append(np.concatenate([p0[5::15][:4, :3, :4], p1[15::15][:4, :3, :4]], 0))
  out['vv_poses'] = np.stack(sel)  # [3, 8, 3, 4]
  path = os.path.join(HERE, 'virtual_views.npz')
  np.savez_compressed(path, **out)
  print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
