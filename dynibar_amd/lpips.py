"""Masked LPIPS of the reference's evaluation loop (eval_nvidia.py:250-263, :289-291, :402-457) on the gfx950 kernels: LPIPS v0.1 with
``net='alex'``, ``model='net-lin'`` (csrc/dyn_lpips.h).

    net = LPIPS.from_files('alexnet-owt-7be5be79.pth', 'alex.pth')           # torchvision's alexnet, the lpips package's weights/v0.1/alex.pth
    net(pred, target)                                                       # the standard LPIPS of two [H, W, 3] images in [0, 1]
    metrics.nvidia_frame_metrics(pred, target, dynamic_mask, lpips=net)     # adds lpips, dynamic_lpips, static_lpips

No weights ship with the package.  ``LPIPS(alexnet_state_dict, lin_state_dict)`` takes the two state dicts the user already has: the keys
``features.{0,3,6,8,10}.{weight,bias}`` of torchvision's ``alexnet`` (further keys, the classifier's, are ignored) and
``lin{0..4}.model.1.weight`` ``[1, C, 1, 1]`` of the ``lpips`` package.  Missing keys, wrong shapes, non-finite values and negative lin weights
raise ``ValueError``.  The weights are packed once per device.

The contract -- preparation as ``metrics.frame_sums``, ``im2tensor``, the scaling layer, AlexNet's five taps, unit-normalised differences
weighted by ``lin``, and per mask ``lpips = sum_l (sum d_l m_l) / (sum m_l)`` with the mask's channel 0 resized to each tap by nearest
neighbour (``src = (dst * n_in) // n_out``; a tap where the mask is empty contributes 0) -- is stated in DESIGN.md section 4.19.  With
``mask=None`` or all ones this is the standard LPIPS, a plain spatial mean.  NOT VERIFIED: the script's ``models`` package is NSFF's
modified copy of LPIPS, and neither it nor its masked form nor the pretrained weights were available when this was written; the masked
average is this package's stated form.

Images are float32 ``[H, W, 3]`` (the target may be uint8), ``H, W >= 31``: the smallest image for which both max-pools have a full window.
There is no CPU fallback: without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, metrics
from ._lib import call, params, stream_of

TAPS = 5
CHANNELS = (64, 192, 384, 256, 256)
FEATURE_INDEX = (0, 3, 6, 8, 10)
_CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
MIN_SIZE = 31
MAX_MASKS = metrics.MAX_MASKS


def tap_sizes(H, W):
  """the five taps' ``(H_l, W_l)`` for an ``H x W`` image"""
  def conv1(n):
    return (n + 4 - 11) // 4 + 1

  def pool(n):
    return (n - 3) // 2 + 1

  s1 = (conv1(H), conv1(W))
  s2 = (pool(s1[0]), pool(s1[1]))
  s3 = (pool(s2[0]), pool(s2[1]))
  return (s1, s2, s3, s3, s3)


def _host_f32(x, name):
  if isinstance(x, torch.Tensor):
    x = x.detach().cpu().numpy()
  x = np.asarray(x)
  if x.dtype.kind != 'f':
    raise ValueError(f'{name} must be a floating-point tensor, got {x.dtype}')
  return np.ascontiguousarray(x, dtype=np.float32)


def lpips_of(rows):
  """one mask's ``[5][2]`` rows (S_l, M_l) -> ``sum_l S_l / M_l``; a tap with M_l = 0 contributes 0"""
  return sum((s / m if m != 0 else 0.0) for s, m in rows)


class LPIPS(object):
  """The packed network.  ``net.frame_sums(...)`` queues one ``dyn_lpips_frame``; ``net(pred, target, mask=None)`` -> a Python float."""

  def __init__(self, alexnet_state_dict, lin_state_dict):
    arrs = []
    for i, shape in zip(FEATURE_INDEX, _CONV_SHAPES):
      for kind, want in (('weight', shape), ('bias', shape[:1])):
        key = f'features.{i}.{kind}'
        if key not in alexnet_state_dict:
          raise ValueError(f'alexnet state dict has no {key!r}')
        a = _host_f32(alexnet_state_dict[key], key)
        if tuple(a.shape) != want:
          raise ValueError(f'{key} has shape {tuple(a.shape)}, torchvision\'s alexnet has {want}')
        if not np.isfinite(a).all():
          raise ValueError(f'{key} has an element that is not finite')
        arrs.append(a.reshape(-1))
    for l, C in enumerate(CHANNELS):
      key = f'lin{l}.model.1.weight'
      if key not in lin_state_dict:
        raise ValueError(f'lin state dict has no {key!r}')
      a = _host_f32(lin_state_dict[key], key)
      if tuple(a.shape) != (1, C, 1, 1):
        raise ValueError(f'{key} has shape {tuple(a.shape)}, LPIPS v0.1 alex has {(1, C, 1, 1)}')
      if not np.isfinite(a).all():
        raise ValueError(f'{key} has an element that is not finite')
      if (a < 0).any():
        raise ValueError(f'{key} has a negative weight: d_l would not be a distance')
      arrs.append(a.reshape(-1))
    self._arrs = arrs
    self._host_blob = None
    self._blobs = {}

  @classmethod
  def from_files(cls, alexnet_path, lin_path):
    """``torch.load`` of torchvision's ``alexnet`` checkpoint and of the lpips package's ``weights/v0.1/alex.pth``"""
    return cls(torch.load(alexnet_path, map_location='cpu'), torch.load(lin_path, map_location='cpu'))

  def _blob(self, device):
    key = str(device)
    if key not in self._blobs:
      if self._host_blob is None:
        n = int(_lib.lib().dyn_lpips_blob_floats())
        blob = np.zeros(n, dtype=np.float32)
        ptrs = (ctypes.c_void_p * len(self._arrs))(*[a.ctypes.data for a in self._arrs])
        try:
          call('dyn_lpips_pack', ptrs, ctypes.c_void_p(blob.ctypes.data), n)
        except RuntimeError as e:
          raise ValueError(str(e)) from None
        self._host_blob = torch.from_numpy(blob)
      self._blobs[key] = self._host_blob.to(device)
    return self._blobs[key]

  def frame_sums(self, pred, target, masks=(), *, apply_valid=False, valid_as_mask0=False, out=None, want_maps=False, want_prepared=False):
    """One ``dyn_lpips_frame`` call on device tensors; no synchronisation, nothing is read back.

    pred float32 ``[H, W, 3]``, target float32 or uint8 ``[H, W, 3]``, masks as ``metrics.frame_sums`` takes them (channel 0 is used).
    -> dict: ``sums`` double ``[M, 5, 2]`` = (S_l, M_l) per mask and tap, mask 0 being the valid mask when ``valid_as_mask0``; with
    ``want_maps`` ``maps``, the five ``d_l`` as double ``[H_l, W_l]`` views of one buffer; with ``want_prepared`` ``prepared`` float32
    ``[2, H, W, 3]``, the scaled pred and target.  ``out``: a contiguous double ``[M, 5, 2]`` tensor on pred's device that receives the sums."""
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
      raise ValueError('frame_sums takes torch tensors (LPIPS.__call__ and metrics.nvidia_frame_metrics also take numpy arrays)')
    if pred.dtype != torch.float32 or pred.dim() != 3 or pred.shape[2] != 3:
      raise ValueError(f'pred must be float32 [H, W, 3], got {str(pred.dtype).replace("torch.", "")} {tuple(pred.shape)}')
    if target.dtype not in (torch.float32, torch.uint8) or tuple(target.shape) != tuple(pred.shape):
      raise ValueError(f'target must be float32 or uint8 {tuple(pred.shape)}, got {str(target.dtype).replace("torch.", "")} {tuple(target.shape)}')
    H, W = int(pred.shape[0]), int(pred.shape[1])
    if H < MIN_SIZE or W < MIN_SIZE:
      raise ValueError(f'image of {H} x {W}: LPIPS needs at least {MIN_SIZE} x {MIN_SIZE} (both max-pools need a full window)')
    dev = pred.device
    if target.device != dev:
      raise ValueError(f'pred is on {dev}, target on {target.device}')
    pred, target = pred.contiguous(), target.contiguous()
    if isinstance(masks, torch.Tensor):
      if masks.dtype != torch.float32 or masks.dim() != 4 or tuple(masks.shape[1:3]) != (H, W) or masks.shape[3] not in (1, 3) or masks.device != dev:
        raise ValueError(f'stacked masks must be float32 [n, {H}, {W}, 1 or 3] on {dev}, got {tuple(masks.shape)}')
      stacked, C = masks.contiguous(), int(masks.shape[3])
    else:
      stacked, C = metrics._stack_masks(masks, (H, W), dev)
    n_user = 0 if stacked is None else int(stacked.shape[0])
    M = n_user + (1 if valid_as_mask0 else 0)
    if M < 1 or M > MAX_MASKS:
      raise ValueError(f'{M} masks in one call (1..{MAX_MASKS})')
    need = int(_lib.lib().dyn_lpips_workspace_bytes(H, W, M))
    if need == 0:
      raise ValueError(f'frame of {H} x {W} with {M} masks is unsupported (H, W >= {MIN_SIZE}, H*W*4 < 2^31)')
    ws = metrics._scratch((need + 7) // 8, torch.float64, dev)
    if out is None:
      sums = metrics._scratch(M * TAPS * 2, torch.float64, dev).view(M, TAPS, 2)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (M, TAPS, 2) or not out.is_contiguous()
          or out.device != dev):
      raise ValueError(f'out must be a contiguous float64 tensor [{M}, {TAPS}, 2] on {dev}')
    else:
      sums = out
    res = dict(sums=sums)
    flat = prepared = None
    if want_maps:
      sizes = tap_sizes(H, W)
      flat = metrics._scratch(sum(h * w for h, w in sizes), torch.float64, dev)
      res['maps'], at = [], 0
      for h, w in sizes:
        res['maps'].append(flat[at:at + h * w].view(h, w))
        at += h * w
    if want_prepared:
      prepared = res['prepared'] = metrics._scratch(2 * H * W * 3, torch.float32, dev).view(2, H, W, 3)
    p = params('DynLpipsParams', H=H, W=W, M=M, blob=metrics._p(self._blob(dev)), pred=metrics._p(pred), target=metrics._p(target),
               target_is_u8=1 if target.dtype == torch.uint8 else 0, masks=metrics._p(stacked), mask_stride=H * W * C, mask_channels=C,
               apply_valid=1 if apply_valid else 0, valid_as_mask0=1 if valid_as_mask0 else 0, maps=metrics._p(flat), prepared=metrics._p(prepared),
               workspace=metrics._p(ws), workspace_bytes=need)
    call('dyn_lpips_frame', p, metrics._p(sums), stream_of(pred))
    return res

  def __call__(self, pred, target, mask=None):
    """LPIPS of two images (numpy arrays or tensors, on the host or a HIP device) under ``mask`` (None: the plain spatial mean) -> float.
    One device-to-host copy."""
    s = metrics._pair(pred, target)
    if len(s) == 3 and (s[0] < MIN_SIZE or s[1] < MIN_SIZE):
      raise ValueError(f'images of {s[0]} x {s[1]}: LPIPS needs at least {MIN_SIZE} x {MIN_SIZE} (both max-pools need a full window)')
    dev = metrics._device_of(pred, target, mask)
    a, b = metrics._image(pred, 'pred', dev), metrics._image(target, 'target', dev, allow_u8=True)
    if mask is None:
      mask = torch.ones((a.shape[0], a.shape[1], 1), dtype=torch.float32, device=dev)
    rows = self.frame_sums(a, b, [mask])['sums'].cpu().tolist()[0]
    return float(lpips_of(rows))
