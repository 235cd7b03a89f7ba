"""The metrics of the reference's evaluation loop (eval_nvidia.py:201-247, :380-457) on the gfx950 kernels; LPIPS is dynibar_amd/lpips.py.

    from eval_nvidia import calculate_psnr, calculate_ssim   ->   from dynibar_amd.metrics import calculate_psnr, calculate_ssim
    numbers = nvidia_frame_metrics(ret['outputs_fine_ref']['rgb'], gt_uint8_or_float, dynamic_mask, lpips=net)   # replaces :383-457

One ``dyn_frame_metrics`` call (csrc/dyn_metrics.h: k_metrics_tile, k_metrics_finish) prepares the frame -- the valid mask
``sum(rgb, -1) > 1e-3`` in float32 in numpy's order of addition, ``float32(uint8) / 255``, both images times the mask, all bit-exact against
numpy -- forms the SSIM map of ``skimage.metrics.structural_similarity`` as the script calls it (7 x 7 uniform window, ``reflect`` boundary,
sample covariance, per channel, ``full=True``) and adds ``sum((a - b)^2 m)``, ``sum(S m)``, ``sum(m)`` for up to 8 masks, in double and in a fixed
order: the numbers are reproducible bit for bit, and a mask's sums do not depend on the other masks of the call.  The divisions and
``10 * log10(1 / mse)`` are done on the host in Python floats from those sums with the reference's expressions.  Per frame: two kernel
launches and ONE device-to-host copy (the ``[M, 3]`` doubles); nothing else synchronises.

``data_range``.  The reference passes float32 images in [0, 1] and no ``data_range``.  The skimage versions that still accept its
``multichannel=True`` take the range of a float image from the dtype (-1 ... 1), i.e. R = 2, not 1 -- from the skimage sources as
remembered: skimage was not available when this was written and the default has NOT been checked against it, nor has the equality of this
map with skimage's own output.  So ``data_range`` is a keyword everywhere and the reference-shaped entries default to
``REFERENCE_DATA_RANGE = 2.0``; pass ``data_range=1.0`` for the usual SSIM of [0, 1] images.

Inputs are numpy arrays or torch tensors on the host or on a HIP device; host inputs are uploaded (a rendered frame is a host tensor by
``render_image``'s output contract: 1.8 MB).  Images are float32 ``[H, W, 3]`` (the target of ``nvidia_frame_metrics`` may be uint8), masks
float32 or bool ``[H, W, 3]``, ``[H, W, 1]`` or ``[H, W]``, ``H, W >= 7``.  Limits raise ``ValueError``.  There is no CPU fallback: without the
library or a device these functions raise.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, params, stream_of
from .train_static import POISON_SCRATCH

REFERENCE_DATA_RANGE = 2.0  # what skimage is believed to derive for the reference's float32 images; unverified (module docstring)
MAX_MASKS = 8


def _device_of(*xs):
  """the one HIP device the call runs on: that of the device tensors among the inputs (they must agree), else the current device"""
  devs = {x.device for x in xs if isinstance(x, torch.Tensor) and x.device.type != 'cpu'}
  if len(devs) > 1:
    raise ValueError('inputs are on different devices: ' + ', '.join(sorted(str(d) for d in devs)))
  if devs:
    dev = devs.pop()
    if dev.type != 'cuda':
      raise ValueError(f'dynibar_amd.metrics needs tensors on the host or on a HIP device (cuda:N); got {dev}')
    return dev
  if not _lib._REQUIRE_DEVICE:
    return torch.device('cpu')
  if not torch.cuda.is_available():
    raise RuntimeError('dynibar_amd.metrics needs a HIP device (cuda:N) to run its kernels: there is no CPU fallback')
  return torch.device('cuda', torch.cuda.current_device())


def _tensor(x, what):
  if isinstance(x, np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(x))
  if isinstance(x, torch.Tensor):
    return x.detach()
  raise ValueError(f'{what} must be a numpy array or a torch tensor, got {type(x).__name__}')


def _image(x, what, device, allow_u8=False):
  t = _tensor(x, what)
  ok = (torch.float32, torch.uint8) if allow_u8 else (torch.float32,)
  if t.dtype not in ok:
    raise ValueError(f'{what} must be {" or ".join(str(d).replace("torch.", "") for d in ok)}, got {str(t.dtype).replace("torch.", "")}')
  if t.dim() != 3 or t.shape[2] != 3:
    raise ValueError(f'{what} must be [H, W, 3], got {tuple(t.shape)}')
  if t.shape[0] < 7 or t.shape[1] < 7:
    raise ValueError(f'{what} is {t.shape[0]} x {t.shape[1]}: smaller than the 7 x 7 window of the SSIM')
  return t.to(device).contiguous()


def _mask(x, what, shape, device):
  """-> float32 [H, W, C] on the device, C = 1 or 3"""
  t = _tensor(x, what)
  if t.dtype == torch.bool:
    t = t.to(device).to(torch.float32)
  elif t.dtype != torch.float32:
    raise ValueError(f'{what} must be float32 or bool, got {str(t.dtype).replace("torch.", "")}')
  H, W = shape[0], shape[1]
  if t.dim() == 2:
    t = t[:, :, None]
  if t.dim() != 3 or tuple(t.shape[:2]) != (H, W) or t.shape[2] not in (1, 3):
    raise ValueError(f'{what} must be [{H}, {W}, 3], [{H}, {W}, 1] or [{H}, {W}], got {tuple(x.shape)}')
  return t.to(device)


def _stack_masks(masks, shape, device):
  """masks of one call -> ([n, H, W, C] float32 contiguous, C): one channel count for the call (a 1-channel mask is expanded next to a 3-channel one)"""
  ms = [_mask(m, f'mask {i}', shape, device) for i, m in enumerate(masks)]
  if not ms:
    return None, 1
  C = max(m.shape[2] for m in ms)
  return torch.stack([m.expand(shape[0], shape[1], C) for m in ms]).contiguous(), C


def _scratch(n, dtype, device):
  t = torch.empty((n,), dtype=dtype, device=device)
  if POISON_SCRATCH:  # (train_static.py) under test the kernels must fill what they later read
    t.fill_(float('nan'))
  return t


def _p(t):
  return None if t is None else ctypes.c_void_p(t.data_ptr())


def frame_sums(pred, target, masks=(), *, data_range, apply_valid=False, valid_as_mask0=False, want_map=False, want_valid=False,
               want_prepared=False, out=None):
  """One ``dyn_frame_metrics`` call on device tensors; no synchronisation, nothing is read back.

  pred float32 ``[H, W, 3]``, target float32 or uint8 ``[H, W, 3]``, masks a sequence of float32 ``[H, W, C]`` (or one stacked ``[n, H, W, C]``
  tensor) on pred's device.  -> dict: ``sums`` double ``[M, 3]`` = (sum (a - b)^2 m, sum S m, sum m) per mask, mask 0 being the valid mask when
  ``valid_as_mask0``; on request ``ssim_map`` double ``[H, W, 3]``, ``valid`` uint8 ``[H, W]``, ``pred`` / ``target`` float32 (the prepared images).
  ``out``: a contiguous double ``[M, 3]`` tensor on pred's device (a row block of a larger table, say) that receives the sums and is returned
  as ``sums``; None allocates one."""
  H, W = int(pred.shape[0]), int(pred.shape[1])
  dev = pred.device
  if isinstance(masks, torch.Tensor):
    stacked, C = masks, int(masks.shape[3])
  else:
    stacked, C = _stack_masks(masks, (H, W), dev)
  n_user = 0 if stacked is None else int(stacked.shape[0])
  M = n_user + (1 if valid_as_mask0 else 0)
  if M < 1 or M > MAX_MASKS:
    raise ValueError(f'{M} masks in one call (1..{MAX_MASKS})')
  R = float(data_range)
  if not (R > 0.0 and math.isfinite(R)):
    raise ValueError(f'data_range must be positive and finite, got {data_range!r}')
  need = int(_lib.lib().dyn_frame_metrics_workspace_bytes(H, W, M))
  if need == 0:
    raise ValueError(f'frame of {H} x {W} with {M} masks is unsupported (H, W >= 7, H*W*3 < 2^31)')
  ws = _scratch(need // 8, torch.float64, dev)
  if out is None:
    sums = _scratch(M * 3, torch.float64, dev).view(M, 3)
  elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (M, 3) or not out.is_contiguous()
        or out.device != dev):
    raise ValueError(f'out must be a contiguous float64 tensor [{M}, 3] on {dev}')
  else:
    sums = out
  out = dict(sums=sums)
  if want_map:
    out['ssim_map'] = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
  if want_valid:
    out['valid'] = torch.empty((H, W), dtype=torch.uint8, device=dev)
  if want_prepared:
    out['pred'] = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    out['target'] = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
  p = params('DynFrameMetricsParams', H=H, W=W, M=M, pred=_p(pred), target=_p(target), target_is_u8=1 if target.dtype == torch.uint8 else 0,
             masks=_p(stacked), mask_stride=H * W * C, mask_channels=C, apply_valid=1 if apply_valid else 0,
             valid_as_mask0=1 if valid_as_mask0 else 0, data_range=R, ssim_map=_p(out.get('ssim_map')), valid=_p(out.get('valid')),
             pred_out=_p(out.get('pred')), target_out=_p(out.get('target')), workspace=_p(ws), workspace_bytes=need)
  call('dyn_frame_metrics', p, _p(out['sums']), stream_of(pred))
  return out


def _pair(img1, img2, allow_u8=False):
  s1, s2 = getattr(img1, 'shape', None), getattr(img2, 'shape', None)
  if s1 is None or s2 is None or tuple(s1) != tuple(s2):
    raise ValueError('Input images must have the same dimensions.')
  return s1


def _psnr_of(sse, msum):
  """calculate_psnr's last lines (eval_nvidia.py:218-225) on the device's double sums"""
  num_valid = msum + 1e-8
  mse = sse / num_valid
  if mse == 0:
    return 0  # float('inf')
  return 10 * math.log10(1.0 / mse)


def _ssim_of(ssum, msum):
  """calculate_ssim's last lines (eval_nvidia.py:245-247)"""
  num_valid = msum + 1e-8
  return ssum / num_valid


def _one_mask(img1, img2, mask, data_range):
  _pair(img1, img2)
  dev = _device_of(img1, img2, mask)
  a, b = _image(img1, 'img1', dev), _image(img2, 'img2', dev)
  sums = frame_sums(a, b, [mask], data_range=data_range)['sums']
  return sums.cpu().tolist()[0]  # the one device-to-host copy


def calculate_psnr(img1, img2, mask):
  """eval_nvidia.calculate_psnr: ``10 log10(1 / mse)``, ``mse = sum((img1 - img2)^2 mask) / (sum(mask) + 1e-8)``; 0 (not infinity) when the
  masked squared error is exactly 0, as the reference returns it."""
  sse, _, msum = _one_mask(img1, img2, mask, 1.0)
  return _psnr_of(sse, msum)


def calculate_ssim(img1, img2, mask, *, data_range=REFERENCE_DATA_RANGE):
  """eval_nvidia.calculate_ssim: ``sum(ssim_map mask) / (sum(mask) + 1e-8)`` with the uncropped map of ``structural_similarity``.
  ``data_range`` defaults to what skimage is believed to use for the reference's call (unverified: see the module docstring)."""
  _, ssum, msum = _one_mask(img1, img2, mask, data_range)
  return _ssim_of(ssum, msum)


def structural_similarity(im1, im2, *, data_range, full=False):
  """``skimage.metrics.structural_similarity(im1, im2, channel_axis=-1, data_range=..., full=...)`` for float32 ``[H, W, 3]`` images with the
  defaults the reference uses: the mean of the map cropped by 3 pixels (the masked mean under an interior mask), and with ``full`` the
  whole map as a float64 numpy array."""
  _pair(im1, im2)
  dev = _device_of(im1, im2)
  a, b = _image(im1, 'im1', dev), _image(im2, 'im2', dev)
  H, W = a.shape[0], a.shape[1]
  inner = torch.zeros((1, H, W, 1), dtype=torch.float32, device=dev)
  inner[:, 3:H - 3, 3:W - 3] = 1.0
  out = frame_sums(a, b, inner, data_range=data_range, want_map=full)
  _, ssum, _ = out['sums'].cpu().tolist()[0]
  mssim = ssum / (3 * (H - 6) * (W - 6))
  return (mssim, out['ssim_map'].cpu().numpy()) if full else mssim


def nvidia_frame_metrics(pred_rgb, target, dynamic_mask, *, data_range=REFERENCE_DATA_RANGE, lpips=None):
  """eval_nvidia.py:380-457 for one frame.  pred_rgb float32 ``[H, W, 3]`` (``ret['outputs_fine_ref']['rgb']``), target float32 in
  [0, 1] or uint8 (the resized ground truth before or after ``/ 255``), dynamic_mask ``[H, W, 3]`` or ``[H, W]`` weights (the resized mv_mask).
  Both images are multiplied by the valid mask; the masks valid, dynamic and 1 - dynamic (the static mask is not multiplied by valid: the
  reference does not) are evaluated in one ``dyn_frame_metrics`` call and the nine sums come back in one copy.
  ``lpips``: a ``dynibar_amd.lpips.LPIPS`` network; one ``dyn_lpips_frame`` call then evaluates the same three masks (H, W >= 31) and its table
  comes back in the same copy.  None: no LPIPS, the numbers and their bits are those of the call without the keyword.
  -> dict of Python floats: psnr, ssim, dynamic_psnr, dynamic_ssim, static_psnr, static_ssim, valid_fraction, and with a network lpips,
  dynamic_lpips, static_lpips."""
  _pair(pred_rgb, target)
  dev = _device_of(pred_rgb, target, dynamic_mask)
  a, b = _image(pred_rgb, 'pred_rgb', dev), _image(target, 'target', dev, allow_u8=True)
  H, W = a.shape[0], a.shape[1]
  dyn = _mask(dynamic_mask, 'dynamic_mask', (H, W), dev)
  masks = torch.stack([dyn, 1 - dyn]).contiguous()  # (:444)
  if lpips is None:
    sums = frame_sums(a, b, masks, data_range=data_range, apply_valid=True, valid_as_mask0=True)['sums']
    rows, taps = sums.cpu().tolist(), None  # the one device-to-host copy of the frame
  else:
    both = _scratch(9 + 30, torch.float64, dev)  # [3, 3] of dyn_frame_metrics, then [3, 5, 2] of dyn_lpips_frame: one copy
    frame_sums(a, b, masks, data_range=data_range, apply_valid=True, valid_as_mask0=True, out=both[:9].view(3, 3))
    lpips.frame_sums(a, b, masks, apply_valid=True, valid_as_mask0=True, out=both[9:].view(3, 5, 2))
    host = both.cpu()  # the one device-to-host copy of the frame
    rows, taps = host[:9].view(3, 3).tolist(), host[9:].view(3, 5, 2).tolist()
  out = {}
  for name, (sse, ssum, msum) in zip(('', 'dynamic_', 'static_'), rows):
    out[name + 'psnr'] = _psnr_of(sse, msum)
    out[name + 'ssim'] = _ssim_of(ssum, msum)
  out['valid_fraction'] = rows[0][2] / (3 * H * W)
  if taps is not None:
    from . import lpips as lpips_mod
    for name, t in zip(('', 'dynamic_', 'static_'), taps):
      out[name + 'lpips'] = float(lpips_mod.lpips_of(t))
  return out
