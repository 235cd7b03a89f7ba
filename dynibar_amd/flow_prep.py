"""Flow supervision on the gfx950 kernels: from raw optical flow to the ``flows`` / ``flow_masks`` a ``DeviceScene`` takes (csrc/dyn_flowprep.h).

    flow_utils.warp_flow(img, flow)  (cv2.remap)                   ->   flow_prep.warp_flow(img, flow)
    cv2.resize(flow, (w, h)); flow *= ratio                        ->   flow_prep.resize_flow(flow, (w, h))
    the forward-backward check of a preprocessing script          ->   flow_prep.consistency_masks(flows)
    ... with the epipolar error and a geometric motion vote       ->   flow_prep.supervision(flows, intrinsics, poses)
    a host loop of 6 N warps that writes flow_i{1,2,3}/*.npz       ->   python -m dynibar_amd.flow_prep --raw_dir R --out_dir D

A flow network gives ``flow`` only; the ``mask`` half of ``flow_i{1,2,3}/%05d_{fwd,bwd}.npz`` (monocular.py:91-112) comes from a forward-backward
consistency check: the flow of frame i to frame i + o, plus the flow of frame i + o back to frame i sampled where the first one lands, must
nearly cancel: ``|f + w| < alpha1 * (|f| + |w|) + alpha2``.  ``alpha1 = alpha2 = 0.5`` are this module's defaults and they are parameters: NO CLAIM
is made about the values any upstream preprocessing script uses.  The same flows and the scene's cameras give the Sampson distance of every
flow vector to its epipolar line (``epi``), and a vote over the six offsets gives the geometric half of a motion mask (``motion``: consistent
flow that leaves its epipolar line by more than ``epi_thresh`` pixels for at least ``min_votes`` offsets).

The contract (include/dynibar_hip.h: flow supervision) is IEEE operations in a stated order; tests/flow_prep_cases.py restates it in numpy and the
kernels reproduce the restatement bit for bit.  ``subpixel=32`` restates ``cv2.remap`` as the maintainers know it -- coordinates in 1/32-pixel
fixed point rounded with rint, a constant border applied per tap -- and cv2 was not available when this was written: that ``warp_flow`` returns
what ``cv2.remap`` returns is BELIEVED, NOT VERIFIED against cv2 (``ingest.py`` says the same of ``cv2.resize``).  ``subpixel=0`` samples at the
exact coordinates.

Inputs are numpy arrays or torch tensors, on the host (uploaded to ``device``, default the current HIP device) or already on a HIP device;
results are device tensors.  ``size`` is ``(width, height)``.  Bad arguments raise ``ValueError``; there is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import call, stream_of
from .ingest import _device, _p, _size, _tensor
from .view_selection import FLOW_OFFSETS

DEFAULT_ALPHA = 0.5


def _subpixel(subpixel):
  if subpixel not in (0, 32):
    raise ValueError(f'subpixel={subpixel!r} must be 32 (fixed-point coordinates, as cv2.remap is believed to work) or 0 (exact coordinates)')
  return int(subpixel)


def _result(out, shape, dtype, dev, what):
  """a fresh contiguous tensor, or the caller's ``out``, which must be one on the device"""
  if out is None:
    return torch.empty(shape, dtype=dtype, device=dev)
  if not isinstance(out, torch.Tensor) or out.dtype != dtype or out.device != dev:
    raise ValueError(f'{what}: out must be a {str(dtype).replace("torch.", "")} tensor on {dev}')
  if tuple(out.shape) != tuple(shape) or not out.is_contiguous():
    raise ValueError(f'{what}: out must be a contiguous {list(shape)}, got {list(out.shape)}')
  return out


def resize_flow(raw, size, out=None, device=None):
  """A raw flow field at another size: float32 ``[Hs, Ws, 2]`` or ``[B, Hs, Ws, 2]`` -> the same form at ``size = (width, height)``.  Each channel
  is resized as ``ingest.resize_linear`` resizes a plane, then ``u`` is multiplied by ``float32(width / Ws)`` and ``v`` by ``float32(height / Hs)``
  (the ratio formed in double and rounded once: ``flow *= ratio`` on a float32 numpy array).  Equal sizes are a copy."""
  dev = _device(device, raw, out)
  t = _tensor(raw, 'raw', (torch.float32,), dev)
  if t.dim() not in (3, 4) or t.shape[-1] != 2 or min(t.shape) < 1:
    raise ValueError(f'raw must be float32 [Hs, Ws, 2] or [B, Hs, Ws, 2], got {list(t.shape)}')
  t4 = t if t.dim() == 4 else t[None]
  B, Hs, Ws, _ = (int(v) for v in t4.shape)
  Wd, Hd = _size(size)
  if Hs * Ws >= 2 ** 31 or Hd * Wd >= 2 ** 31:
    raise ValueError(f'resize_flow: {Hs} x {Ws} -> {Hd} x {Wd} is too large (H*W < 2^31)')
  shape = (B, Hd, Wd, 2) if t.dim() == 4 else (Hd, Wd, 2)
  o = _result(out, shape, torch.float32, dev, 'resize_flow')
  if o.data_ptr() == t4.data_ptr():
    raise ValueError('resize_flow: out must not be the input')
  call('dyn_flow_resize', B, Hs, Ws, Hd, Wd, _p(t4), _p(o), stream_of(t4))
  return o


def warp_flow(img, flow, subpixel=32, out=None, device=None):
  """``flow_utils.warp_flow(img, flow)``: ``cv2.remap(img, flow + pixel grid, None, cv2.INTER_LINEAR, borderMode=cv2.BORDER_CONSTANT)``.
  ``flow`` float32 ``[H, W, 2]`` with ``img`` float32 ``[H, W]`` or ``[H, W, C]``; or ``flow`` ``[B, H, W, 2]`` with ``img`` ``[B, H, W]`` or
  ``[B, H, W, C]``; C in 1..4 -> float32 of ``img``'s form.  ``subpixel=32``: OpenCV's 1/32-pixel fixed-point coordinates (believed, not
  verified against cv2); ``subpixel=0``: exact coordinates."""
  sub = _subpixel(subpixel)
  dev = _device(device, img, flow, out)
  f = _tensor(flow, 'flow', (torch.float32,), dev)
  i = _tensor(img, 'img', (torch.float32,), dev)
  if f.dim() not in (3, 4) or f.shape[-1] != 2 or min(f.shape) < 1:
    raise ValueError(f'flow must be float32 [H, W, 2] or [B, H, W, 2], got {list(f.shape)}')
  lead = tuple(f.shape[:-1])
  if tuple(i.shape) == lead:
    C = 1
  elif i.dim() == f.dim() and tuple(i.shape[:-1]) == lead:
    C = int(i.shape[-1])
  else:
    raise ValueError(f'img must be float32 {list(lead)} or {list(lead)} + [C] for a flow of {list(f.shape)}, got {list(i.shape)}')
  if not 1 <= C <= 4:
    raise ValueError(f'img must have 1 to 4 channels, got {C}')
  H, W = int(f.shape[-3]), int(f.shape[-2])
  B = int(f.shape[0]) if f.dim() == 4 else 1
  if H * W >= 2 ** 31:
    raise ValueError(f'warp_flow: {H} x {W} is too large (H*W < 2^31)')
  o = _result(out, tuple(i.shape), torch.float32, dev, 'warp_flow')
  if o.data_ptr() in (i.data_ptr(), f.data_ptr()):
    raise ValueError('warp_flow: out must be neither input')
  call('dyn_warp_flow', B, H, W, C, _p(i), _p(f), _p(o), sub, stream_of(f))
  return o


def fundamental_matrices(intrinsics, poses):
  """The fundamental matrices of a scene's flow pairs, on the host in float64: ``intrinsics`` ``[N, 3, 3]`` or ``[N, 4, 4]`` (or one matrix for all
  frames), ``poses`` camera-to-world ``[N, 4, 4]`` -> float64 ``[N, 6, 9]``, row-major, in the order of the offsets +1, +2, +3, -1, -2, -3; zeros for
  a pair out of range.  For frame i and frame j = i + o: ``T = inv(c2w_j) @ c2w_i`` with rotation ``R`` and translation ``t``,
  ``F = K_j^-T [t]x R K_i^-1`` divided by its Frobenius norm, so that ``x_j^T F x_i = 0`` for matching pixels (the projector's convention:
  ``pixel ~ K inv(c2w) X``).  A norm of 0 (identical camera centres: no epipolar constraint) leaves F all zeros, which gives ``epi = 0``."""
  c2w = np.asarray(poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else poses, dtype=np.float64)
  K = np.asarray(intrinsics.detach().cpu().numpy() if isinstance(intrinsics, torch.Tensor) else intrinsics, dtype=np.float64)
  if c2w.ndim != 3 or c2w.shape[0] < 1 or c2w.shape[1:] != (4, 4):
    raise ValueError(f'poses must be camera-to-world [N, 4, 4], got {list(c2w.shape)}')
  N = c2w.shape[0]
  if K.ndim == 2:
    K = np.broadcast_to(K, (N,) + K.shape)
  if K.ndim != 3 or K.shape[0] != N or K.shape[1:] not in ((3, 3), (4, 4)):
    raise ValueError(f'intrinsics must be [{N}, 3, 3] or [{N}, 4, 4] (or one such matrix), got {list(K.shape)}')
  Kinv = np.stack([np.linalg.inv(k[:3, :3]) for k in K])
  w2c = np.stack([np.linalg.inv(c) for c in c2w])
  F = np.zeros((N, 6, 9), dtype=np.float64)
  for i in range(N):
    for j, o in enumerate(FLOW_OFFSETS):
      p = i + o
      if not 0 <= p < N:
        continue
      T = w2c[p] @ c2w[i]
      R, t = T[:3, :3], T[:3, 3]
      tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
      f = Kinv[p].T @ tx @ R @ Kinv[i]
      n = np.linalg.norm(f)
      if n > 0 and np.isfinite(n):
        F[i, j] = (f / n).reshape(9)
  return F


def _flows(flows, dev):
  t = _tensor(flows, 'flows', (torch.float32,), dev)
  if t.dim() != 5 or t.shape[1] != 6 or t.shape[4] != 2 or min(t.shape) < 1:
    raise ValueError(f'flows must be float32 [N, 6, H, W, 2] with N, H, W >= 1 (the offsets +1, +2, +3, -1, -2, -3), got {list(t.shape)}')
  N, _, H, W, _ = (int(v) for v in t.shape)
  if H * W >= 2 ** 31 or N >= 2 ** 31:
    raise ValueError(f'flows of {N} frames of {H} x {W} are too large (H*W < 2^31)')
  return t, N, H, W


def _launch(t, N, H, W, F, alpha1, alpha2, sub, epi_thresh, min_votes, masks, epi, motion):
  call('dyn_flow_supervision', N, H, W, _p(t), _p(F), float(alpha1), float(alpha2), sub, float(epi_thresh), int(min_votes), _p(masks), _p(epi),
       _p(motion), stream_of(t))


def _alphas(alpha1, alpha2):
  a1, a2 = float(alpha1), float(alpha2)
  if a1 != a1 or a2 != a2:
    raise ValueError(f'alpha1={alpha1}, alpha2={alpha2}: not a number')
  return a1, a2


def consistency_masks(flows, alpha1=DEFAULT_ALPHA, alpha2=DEFAULT_ALPHA, subpixel=32, device=None):
  """The forward-backward consistency masks of a scene's flows: float32 ``[N, 6, H, W, 2]`` -> uint8 0 / 1 ``[N, 6, H, W]`` on the device, what
  ``DeviceScene`` takes as ``flow_masks``.  A pair whose partner frame is outside the scene, and non-finite flow, give 0."""
  sub = _subpixel(subpixel)
  a1, a2 = _alphas(alpha1, alpha2)
  dev = _device(device, flows)
  t, N, H, W = _flows(flows, dev)
  masks = torch.empty((N, 6, H, W), dtype=torch.uint8, device=dev)
  _launch(t, N, H, W, None, a1, a2, sub, 0.0, 0, masks, None, None)
  return masks


def supervision(flows, intrinsics=None, poses=None, alpha1=DEFAULT_ALPHA, alpha2=DEFAULT_ALPHA, subpixel=32, epi_thresh=1.0, min_votes=2,
                want_epi=True, device=None):
  """Everything the flows of a scene give, in one launch -> a dict of device tensors:

  flow_masks  uint8 ``[N, 6, H, W]``: ``consistency_masks(flows, ...)``, in the layout ``DeviceScene(...)`` and ``DeviceScene.from_decoded`` take
  epi         float32 ``[N, 6, H, W]``: the Sampson distance, in pixels, of every flow vector to the epipolar geometry of its frame pair
              (``fundamental_matrices(intrinsics, poses)``); 0 for a pair out of range and for non-finite flow.  Only with cameras and ``want_epi``.
  motion      uint8 ``[N, H, W]``: 1 where at least ``min_votes`` of the in-range offsets have a consistent flow with ``epi > epi_thresh``: the
              geometric half of a ``dynamic_masks`` file, before ``ingest.motion_mask``'s erosion.  Only with cameras.
  ``intrinsics`` and ``poses`` (host arrays, as ``DeviceScene`` takes them) come together or not at all."""
  sub = _subpixel(subpixel)
  a1, a2 = _alphas(alpha1, alpha2)
  if (intrinsics is None) != (poses is None):
    raise ValueError('epi and motion need the cameras: pass both intrinsics and poses, or neither')
  thresh = float(epi_thresh)
  if thresh != thresh:
    raise ValueError(f'epi_thresh={epi_thresh} is not a number')
  dev = _device(device, flows)
  t, N, H, W = _flows(flows, dev)
  out = dict(flow_masks=torch.empty((N, 6, H, W), dtype=torch.uint8, device=dev))
  F = None
  if poses is not None:
    Fh = fundamental_matrices(intrinsics, poses)
    if Fh.shape[0] != N:
      raise ValueError(f'{Fh.shape[0]} cameras for {N} frames of flow')
    F = torch.from_numpy(Fh)
    F = F.pin_memory().to(dev, non_blocking=True) if dev.type == 'cuda' else F
    if want_epi:
      out['epi'] = torch.empty((N, 6, H, W), dtype=torch.float32, device=dev)
    out['motion'] = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
  _launch(t, N, H, W, F, a1, a2, sub, thresh, int(min_votes), out['flow_masks'], out.get('epi'), out.get('motion'))
  return out


# ---- the command-line tool: python -m dynibar_amd.flow_prep ----------------------------------------------------------------------------
INTERVALS = (1, 2, 3)


def _flow_path(root, interval, index, fwd):
  import os
  return os.path.join(root, 'flow_i%d' % interval, '%05d_%s.npz' % (index, 'fwd' if fwd else 'bwd'))


def read_raw_flows(raw_dir):
  """``raw_dir/flow_i{1,2,3}/%05d_{fwd,bwd}.npz`` (key ``flow``, float32 ``[H, W, 2]``) -> (flows float32 ``[N, 6, H, W, 2]`` in ``DeviceScene``'s
  order, present bool ``[N, 6]``).  N is one more than the largest frame index found; a missing file is a pair out of range (its flow is zero):
  only the files whose partner frame would lie outside the video may be missing."""
  import glob
  import os
  names = [os.path.basename(p) for k in INTERVALS for p in glob.glob(os.path.join(raw_dir, 'flow_i%d' % k, '*_[fb]wd.npz'))]
  if not names:
    raise SystemExit(f'no flow_i{{1,2,3}}/NNNNN_{{fwd,bwd}}.npz under {raw_dir}')
  N = max(int(n[:5]) for n in names) + 1
  flows, present = None, np.zeros((N, 6), dtype=bool)
  for i in range(N):
    for j, o in enumerate(FLOW_OFFSETS):
      path = _flow_path(raw_dir, abs(o), i, o > 0)
      if not os.path.exists(path):
        if 0 <= i + o < N:
          raise SystemExit(f'{path} is missing: frame {i + o} exists, so only a flow that leaves the video may be absent')
        continue
      f = np.load(path)['flow']
      if f.ndim != 3 or f.shape[2] != 2:
        raise SystemExit(f'{path}: flow must be [H, W, 2], got {list(f.shape)}')
      if flows is None:
        flows = np.zeros((N, 6) + f.shape, dtype=np.float32)
      if f.shape != flows.shape[2:]:
        raise SystemExit(f'{path}: flow is {list(f.shape)}, the others are {list(flows.shape[2:])}')
      flows[i, j] = f
      present[i, j] = True
  return flows, present


def read_cameras(path, size):
  """an LLFF ``poses_bounds*.npy`` -> (intrinsics ``[N, 4, 4]``, c2w ``[N, 4, 4]``) for images of ``size = (width, height)``: the focal length of the
  file scales with the width"""
  from . import camera_format
  arr = np.load(path)
  poses = arr[:, :15].reshape(-1, 3, 5).astype(np.float64)
  poses = np.concatenate([poses[:, :, 1:2], -poses[:, :, 0:1], poses[:, :, 2:]], axis=2)  # (the axis order of load_llff_data)
  w, h = size
  poses[:, 2, 4] *= w / poses[:, 1, 4]
  poses[:, 0, 4], poses[:, 1, 4] = h, w
  return camera_format.batch_parse_llff_poses(poses)


def main(argv=None):
  """``python -m dynibar_amd.flow_prep --raw_dir R --out_dir D``: from a flow network's ``R/flow_i{1,2,3}/%05d_{fwd,bwd}.npz`` (key ``flow``) the files
  ``read_optical_flow`` loads, ``D/flow_i{k}/%05d_{fwd,bwd}.npz`` with ``flow`` (float32, resized if ``--size`` differs) and ``mask`` (bool); with
  ``--poses`` also ``D/flow_motion_masks/%d.png`` (0 / 255)."""
  import argparse
  import os
  ap = argparse.ArgumentParser(description='Write the flow files of a monocular scene with their consistency masks (GPU).')
  ap.add_argument('--raw_dir', required=True, help='the folder with flow_i1, flow_i2, flow_i3 as the flow network left them (key flow)')
  ap.add_argument('--out_dir', required=True, help='where flow_i{1,2,3}/NNNNN_{fwd,bwd}.npz with flow and mask are written')
  ap.add_argument('--size', type=int, nargs=2, metavar=('W', 'H'), default=None, help='the size of the scene; default: the size of the raw flow')
  ap.add_argument('--alpha1', type=float, default=DEFAULT_ALPHA)
  ap.add_argument('--alpha2', type=float, default=DEFAULT_ALPHA)
  ap.add_argument('--subpixel', type=int, default=32, choices=(0, 32))
  ap.add_argument('--poses', default=None, help='an LLFF poses_bounds*.npy: also write flow_motion_masks/%%d.png from the epipolar vote')
  ap.add_argument('--epi_thresh', type=float, default=1.0)
  ap.add_argument('--min_votes', type=int, default=2)
  a = ap.parse_args(argv)
  raw, present = read_raw_flows(a.raw_dir)
  N, _, Hs, Ws, _ = raw.shape
  dev = _device(None)
  flows = torch.from_numpy(raw).to(dev)
  if a.size is not None and tuple(a.size) != (Ws, Hs):
    flows = resize_flow(flows.view(N * 6, Hs, Ws, 2), tuple(a.size), device=dev).view(N, 6, a.size[1], a.size[0], 2)
  H, W = int(flows.shape[2]), int(flows.shape[3])
  cams = read_cameras(a.poses, (W, H)) if a.poses else (None, None)
  if a.poses and cams[1].shape[0] != N:
    raise SystemExit(f'{a.poses} holds {cams[1].shape[0]} cameras, the flow files {N} frames')
  res = supervision(flows, cams[0], cams[1], alpha1=a.alpha1, alpha2=a.alpha2, subpixel=a.subpixel, epi_thresh=a.epi_thresh, min_votes=a.min_votes,
                    want_epi=False, device=dev)
  flows_h, masks_h = flows.cpu().numpy(), res['flow_masks'].cpu().numpy()
  for k in INTERVALS:
    os.makedirs(os.path.join(a.out_dir, 'flow_i%d' % k), exist_ok=True)
  for i in range(N):
    for j, o in enumerate(FLOW_OFFSETS):
      if present[i, j]:
        np.savez(_flow_path(a.out_dir, abs(o), i, o > 0), flow=flows_h[i, j], mask=masks_h[i, j].astype(bool))
  if a.poses:
    from PIL import Image
    os.makedirs(os.path.join(a.out_dir, 'flow_motion_masks'), exist_ok=True)
    motion = res['motion'].cpu().numpy()
    for i in range(N):
      Image.fromarray(motion[i] * np.uint8(255)).save(os.path.join(a.out_dir, 'flow_motion_masks', '%d.png' % i))
  return 0


if __name__ == '__main__':
  raise SystemExit(main())
