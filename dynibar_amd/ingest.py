"""Scene preparation on the gfx950 kernels: from decoded files to the arrays a ``DeviceScene`` takes (csrc/dyn_ingest.h).

    cv2.resize(img, (w, h), interpolation=cv2.INTER_AREA)      ->   ingest.resize_area(img, (w, h))
    cv2.resize(disp, (w, h), interpolation=cv2.INTER_LINEAR)   ->   ingest.resize_linear(disp, (w, h))
    cv2.resize(mask, (w, h), interpolation=cv2.INTER_NEAREST)  ->   ingest.resize_nearest(mask, (w, h))
    skimage.morphology.erosion(m, skimage.morphology.disk(r))  ->   ingest.erode_disk(m, r)
    np.percentile(depth, 5), np.percentile(depth, 95)          ->   ingest.depth_bounds(depth)
    monocular.py:168-203 (the motion mask of a frame)          ->   ingest.motion_mask(raw_u8, (w, h), erosion_radius)
    monocular.py:173-181, :204 (the static mask)               ->   ingest.static_mask(raw_u8, (w, h))
    save_monocular_cameras.py:72, :93-95 and monocular.py:162  ->   ingest.disparity(depth, (w, h), scale)
    python save_monocular_cameras.py --data_dir D --cvd_dir C  ->   python -m dynibar_amd.ingest --data_dir D --cvd_dir C
    cv2.resize(img_1, (w, h), interpolation=cv2.INTER_AREA)    ->   ingest.resize_area_f32(img_1, (w, h))  (float32: shrinking and enlarging)
    render_source_vv.py:253-330 for every frame of a scene     ->   ingest.build_virtual_views(img_1, depth, K_t, cam_c2w, (w, h))
    python render_source_vv.py --data_dir D --cvd_dir C        ->   python -m dynibar_amd.ingest --data_dir D --cvd_dir C --virtual_views

``size`` is ``(width, height)``, the order of cv2's ``dsize``.  The path from decoded files to a resident scene needs numpy, PIL and this
package only: ``prepare_monocular`` runs the loader's chains for every frame of a scene and ``DeviceScene.from_decoded`` hands the result to
the constructor; no image data goes back to the host (the constructor reads back one boolean per mask store, its 0 / 1 check).

The contracts (include/dynibar_hip.h: scene preparation) restate OpenCV's and skimage's algorithms as the maintainers know them.  Neither
library was available when this was written: that these functions return what ``cv2.resize`` and ``skimage.morphology.erosion`` return is
BELIEVED, NOT VERIFIED against cv2 / skimage.  What the tests pin is the stated contract and, per operation, an independent definition (a
float64 box average, ``F.interpolate``, scipy's binary erosion, ``np.percentile``).

Inputs are numpy arrays or torch tensors, on the host (uploaded to ``device``, default the current HIP device) or already on a HIP device;
results are device tensors.  With device inputs nothing synchronises.  Bad arguments raise ``ValueError``; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import virtual_views as vvmod
from ._lib import call, stream_of

MAX_RADIUS = 15
BASE_HEIGHT = 288     # the height at which the loader erodes the motion mask (monocular.py:184-188) and save_monocular_cameras.py's FINAL_H
DEFAULT_BATCH = 8     # frames per launch in prepare_monocular: bounds the full-resolution bytes resident at a time
_TABLES = {}          # (source size, destination size, device) -> the decimation table of an axis on that device


def _p(t):
  return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- what depends on sizes alone (host) ----------------------------------------------------------------------------------------------
def axis_scale(s, d):
  return 1.0 / (float(d) / s)


def is_integer_scale(scale):
  return abs(scale - int(scale)) < 2.220446049250313e-16  # DBL_EPSILON


def area_table(s, d):
  """The decimation table of one axis of ``INTER_AREA`` (include/dynibar_hip.h: dyn_resize_area_u8), built in double and rounded to float32.
  -> (count int32 [d], idx int32 [d, K], weight float32 [d, K]); entries past ``count[i]`` are zero."""
  s, d = int(s), int(d)
  if not 1 <= d <= s:
    raise ValueError(f'an INTER_AREA axis shrinks: {s} -> {d}')
  scale = axis_scale(s, d)
  rows = []
  for i in range(d):
    f1 = i * scale
    f2 = f1 + scale
    cell = min(scale, s - f1)
    s1 = math.ceil(f1)
    s2 = min(math.floor(f2), s - 1)
    s1 = min(s1, s2)
    row = []
    if s1 - f1 > 1e-3:
      row.append((s1 - 1, (s1 - f1) / cell))
    for k in range(s1, s2):
      row.append((k, 1.0 / cell))
    if f2 - s2 > 1e-3:
      row.append((s2, min(min(f2 - s2, 1.0), cell) / cell))
    rows.append(row)
  K = max(1, max(len(r) for r in rows))
  count = np.zeros((d,), np.int32)
  idx = np.zeros((d, K), np.int32)
  w = np.zeros((d, K), np.float32)
  for i, row in enumerate(rows):
    count[i] = len(row)
    for k, (j, a) in enumerate(row):
      idx[i, k] = j
      w[i, k] = np.float32(a)
  return count, idx, w


def percentile_plan(n, q):
  """What ``np.percentile(x, q)`` of n float32 values by the ``linear`` method derives from n and q alone (numpy/lib/_function_base_impl.py:
  percentile, _quantile, _get_indexes, _get_gamma), in numpy's own operations and dtypes: a scalar ``q`` divided by ``np.float32(100)`` stays
  float32 and so do the virtual index, the weight and the result; a sequence becomes a float64 array and the result float64.
  -> (rank int32 [len(q), 2]: the order statistics below and above each percentile; weight [len(q)]: float32 or float64)."""
  n = int(n)
  if n < 1:
    raise ValueError(f'a percentile of {n} values')
  scalar = np.ndim(q) == 0
  qs = np.true_divide(q, np.float32(100))  # (percentile's own division; the divisor takes the data's dtype)
  if not scalar:
    qs = np.asanyarray(qs)
  if not (np.all(qs >= 0) and np.all(qs <= 1)):
    raise ValueError('Percentiles must be in the range [0, 100]')
  virtual = np.asanyarray((n - 1) * qs)
  previous = np.asanyarray(np.floor(virtual))
  nxt = np.asanyarray(previous + 1)
  above = virtual >= n - 1
  previous[above] = -1
  nxt[above] = -1
  previous, nxt = previous.astype(np.intp), nxt.astype(np.intp)
  weight = np.asanyarray(np.asanyarray(virtual - previous), dtype=virtual.dtype)
  rank = np.stack([np.atleast_1d(previous), np.atleast_1d(nxt)], axis=1)
  rank = np.where(rank < 0, rank + n, rank).astype(np.int32)
  return rank, np.atleast_1d(weight)


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def _device(device, *xs):
  devs = {x.device for x in xs if isinstance(x, torch.Tensor) and x.device.type != 'cpu'}
  if device is not None:
    d = torch.device(device)
    devs.add(torch.device('cuda', torch.cuda.current_device()) if d.type == 'cuda' and d.index is None else d)
  if len(devs) > 1:
    raise ValueError('inputs are on different devices: ' + ', '.join(sorted(str(d) for d in devs)))
  if devs:
    dev = devs.pop()
    if dev.type != 'cuda' and _lib._REQUIRE_DEVICE:
      raise ValueError(f'dynibar_amd.ingest needs a HIP device (cuda:N), got {dev}: there is no CPU fallback')
    return dev
  if not _lib._REQUIRE_DEVICE:
    return torch.device('cpu')
  if not torch.cuda.is_available():
    raise RuntimeError('dynibar_amd.ingest needs a HIP device (cuda:N) to run its kernels: there is no CPU fallback')
  return torch.device('cuda', torch.cuda.current_device())


def _tensor(x, what, dtypes, device):
  if isinstance(x, np.ndarray):
    x = torch.from_numpy(np.ascontiguousarray(x))
  if not isinstance(x, torch.Tensor):
    raise ValueError(f'{what} must be a numpy array or a torch tensor, got {type(x).__name__}')
  if x.dtype not in dtypes:
    raise ValueError(f'{what} must be {" or ".join(str(d).replace("torch.", "") for d in dtypes)}, got {str(x.dtype).replace("torch.", "")}')
  return x.detach().to(device).contiguous()


def _size(size):
  try:
    w, h = (int(v) for v in size)
  except (TypeError, ValueError):
    raise ValueError(f'size must be (width, height), got {size!r}') from None
  if w < 1 or h < 1:
    raise ValueError(f'size must be (width, height), both at least 1, got {size!r}')
  return w, h


def _batched(t, what, layouts):
  """layouts: {ndim: how to reach [B, H, W, C]} -> (the [B, H, W, C] view, a function that gives a result its caller's form)"""
  if not isinstance(t, torch.Tensor):
    raise ValueError(f'{what} must be a torch tensor, got {type(t).__name__}')
  if t.dim() not in layouts:
    raise ValueError(f'{what} must be {" or ".join(layouts[k][0] for k in sorted(layouts))}, got {list(t.shape)}')
  _, to4, back = layouts[t.dim()]
  t4 = to4(t)
  if min(t4.shape) < 1:
    raise ValueError(f'{what} is empty: {list(t.shape)}')
  return t4, back


_IMAGE_LAYOUTS = {2: ('[H, W]', lambda t: t[None, :, :, None], lambda r: r[0, :, :, 0]), 3: ('[H, W, C]', lambda t: t[None], lambda r: r[0]),
                  4: ('[B, H, W, C]', lambda t: t, lambda r: r)}
_PLANE_LAYOUTS = {2: ('[H, W]', lambda t: t[None, :, :, None], lambda r: r[0, :, :, 0]),
                  3: ('[B, H, W]', lambda t: t[:, :, :, None], lambda r: r[:, :, :, 0])}


def _out(out, shape, dtype, device, what):
  """the destination [B, H, W, C] and its pitch in bytes: a fresh tensor, or the caller's ``out``, whose images may be spaced apart (a view
  into a pitched store); within an image it must be contiguous"""
  if out is None:
    out = torch.empty(shape, dtype=dtype, device=device)
  else:
    if not isinstance(out, torch.Tensor) or out.dtype != dtype or out.device != device:
      raise ValueError(f'{what}: out must be a {str(dtype).replace("torch.", "")} tensor on {device}')
    if tuple(out.shape) != tuple(shape):
      raise ValueError(f'{what}: out must hold {list(shape)}, got {list(out.shape)}')
    inner = out[0]
    if not inner.is_contiguous():
      raise ValueError(f'{what}: each image of out must be contiguous')
    if shape[0] > 1 and out.stride(0) < inner.numel():
      raise ValueError(f'{what}: the images of out overlap')
  pitch = (out.stride(0) if shape[0] > 1 else out[0].numel()) * out.element_size()
  return out, int(pitch)


def _device_table(s, d, device):
  key = (int(s), int(d), str(device))
  if key not in _TABLES:
    tabs = [torch.from_numpy(a) for a in area_table(s, d)]
    if device.type == 'cuda':  # through pinned memory: the upload is asynchronous (the pinned block is kept until the copy has run)
      tabs = [t.pin_memory().to(device, non_blocking=True) for t in tabs]
    _TABLES[key] = tabs
  return _TABLES[key]


# ---- the five operations -------------------------------------------------------------------------------------------------------------
def resize_area(images, size, out=None, device=None):
  """``cv2.resize(images, size, interpolation=cv2.INTER_AREA)`` for shrinking: uint8 ``[H, W]``, ``[H, W, C]`` or ``[B, H, W, C]`` with C in
  1, 3, 4 -> uint8 of the same form at ``size = (width, height)``.  ``out``: a uint8 tensor to write into; its images may be spaced apart.
  (float32 images, shrinking or enlarging: ``resize_area_f32``.)"""
  dev = _device(device, images, out)
  t4, back = _batched(_tensor(images, 'images', (torch.uint8,), dev), 'images', _IMAGE_LAYOUTS)
  B, Hs, Ws, C = (int(v) for v in t4.shape)
  Wd, Hd = _size(size)
  if C not in (1, 3, 4):
    raise ValueError(f'images must have 1, 3 or 4 channels, got {C}')
  if Hd > Hs or Wd > Ws:
    raise ValueError(f'resize_area shrinks: {Hs} x {Ws} -> {Hd} x {Wd} enlarges an axis (the reference only shrinks with INTER_AREA)')
  if Hs * Ws * C >= 2 ** 31 or Hd > 65535 or B > 65535:
    raise ValueError(f'{B} images of {Hs} x {Ws} x {C} -> {Hd} x {Wd} are too large (H*W*C < 2^31, at most 65535 rows and images per call)')
  t4 = t4.contiguous()
  o, pitch = _out(None if out is None else _batched(out, 'out', _IMAGE_LAYOUTS)[0], (B, Hd, Wd, C), torch.uint8, dev, 'resize_area')
  if is_integer_scale(axis_scale(Ws, Wd)) and is_integer_scale(axis_scale(Hs, Hd)):
    tx = ty = (None, None, None)
    Kx = Ky = 0
  else:
    tx, ty = _device_table(Ws, Wd, dev), _device_table(Hs, Hd, dev)
    Kx, Ky = int(tx[1].shape[1]), int(ty[1].shape[1])
  call('dyn_resize_area_u8', B, Hs, Ws, C, Hd, Wd, _p(t4), _p(o), pitch, _p(tx[0]), _p(tx[1]), _p(tx[2]), Kx, _p(ty[0]), _p(ty[1]), _p(ty[2]), Ky,
       stream_of(t4))
  return out if out is not None else back(o)


def resize_area_f32(images, size, out=None, device=None):
  """``cv2.resize(images, size, interpolation=cv2.INTER_AREA)`` on float32, shrinking or enlarging: ``[H, W]``, ``[H, W, C]`` or ``[B, H, W, C]``
  with C in 1..4 -> float32 of the same form at ``size = (width, height)``.  Where an axis enlarges OpenCV's INTER_AREA is its two-tap linear
  kernel with area-mode coefficients, on both axes.  The source must be contiguous.  ``out``: a float32 tensor to write into; its images may
  be spaced apart.  (``resize_area`` stays the uint8 form and keeps refusing everything else.)"""
  dev = _device(device, images, out)
  if isinstance(images, torch.Tensor) and not images.is_contiguous():
    raise ValueError(f'images must be contiguous, got strides {list(images.stride())} for {list(images.shape)}')
  if isinstance(images, np.ndarray) and not images.flags.c_contiguous:
    raise ValueError(f'images must be contiguous, got strides {list(images.strides)} for {list(images.shape)}')
  t4, back = _batched(_tensor(images, 'images', (torch.float32,), dev), 'images', _IMAGE_LAYOUTS)
  B, Hs, Ws, C = (int(v) for v in t4.shape)
  Wd, Hd = _size(size)
  if not 1 <= C <= 4:
    raise ValueError(f'float32 images must have 1 to 4 channels, got {C}')
  if Hs * Ws * C * 4 >= 2 ** 31 or Hd * Wd * C * 4 >= 2 ** 31 or Hd > 65535 or B > 65535:
    raise ValueError(f'{B} images of {Hs} x {Ws} x {C} -> {Hd} x {Wd} are too large (H*W*C*4 < 2^31, at most 65535 rows and images per call)')
  o, pitch = _out(None if out is None else _batched(out, 'out', _IMAGE_LAYOUTS)[0], (B, Hd, Wd, C), torch.float32, dev, 'resize_area_f32')
  tx = ty = (None, None, None)
  Kx = Ky = 0
  if Hd <= Hs and Wd <= Ws and not (is_integer_scale(axis_scale(Ws, Wd)) and is_integer_scale(axis_scale(Hs, Hd))):
    tx, ty = _device_table(Ws, Wd, dev), _device_table(Hs, Hd, dev)
    Kx, Ky = int(tx[1].shape[1]), int(ty[1].shape[1])
  call('dyn_resize_area_f32', B, Hs, Ws, C, Hd, Wd, _p(t4), _p(o), pitch, _p(tx[0]), _p(tx[1]), _p(tx[2]), Kx, _p(ty[0]), _p(ty[1]), _p(ty[2]), Ky,
       stream_of(t4))
  return out if out is not None else back(o)


def _linear(x, size, out, device, reciprocal, divisor, what):
  """divisor: None, or the float32 the result is divided by"""
  dev = _device(device, x, out)
  t4, back = _batched(_tensor(x, 'x', (torch.float32,), dev), 'x', _PLANE_LAYOUTS)
  B, Hs, Ws, _ = (int(v) for v in t4.shape)
  Wd, Hd = _size(size)
  if Hs * Ws * 4 >= 2 ** 31 or Hd * Wd * 4 >= 2 ** 31 or Hd > 65535 or B > 65535:
    raise ValueError(f'{what}: {Hs} x {Ws} -> {Hd} x {Wd} is too large')
  t4 = t4.contiguous()
  o, pitch = _out(None if out is None else _batched(out, 'out', _PLANE_LAYOUTS)[0], (B, Hd, Wd, 1), torch.float32, dev, what)
  call('dyn_resize_linear_f32', B, Hs, Ws, Hd, Wd, _p(t4), _p(o), pitch, 1 if reciprocal else 0, 0 if divisor is None else 1,
       0.0 if divisor is None else float(divisor), stream_of(t4))
  return out if out is not None else back(o)


def resize_linear(x, size, out=None, device=None):
  """``cv2.resize(x, size, interpolation=cv2.INTER_LINEAR)``, shrinking or enlarging: float32 ``[H, W]`` or ``[B, H, W]`` -> the same form at
  ``size = (width, height)``.  Non-finite inputs are unspecified."""
  return _linear(x, size, out, device, False, None, 'resize_linear')


def resize_nearest(x, size, below=None, out=None, device=None):
  """``cv2.resize(x, size, interpolation=cv2.INTER_NEAREST)``: uint8 with 1, 3 or 4 channels or float32 with 1 to 3, ``[H, W]``, ``[H, W, C]`` or
  ``[B, H, W, C]`` -> the same form at ``size = (width, height)``.  ``below``: the result is uint8 without the channel axis, 1 where the first
  byte of the pixel is smaller than ``below``, else 0 (``below=255`` is the loader's ``1 - m / 255 > 1e-3`` for a decoded uint8 ``m``)."""
  dev = _device(device, x, out)
  t4, back = _batched(_tensor(x, 'x', (torch.uint8, torch.float32), dev), 'x', _IMAGE_LAYOUTS)
  B, Hs, Ws, C = (int(v) for v in t4.shape)
  Wd, Hd = _size(size)
  px = C * t4.element_size()
  if px not in (1, 3, 4, 8, 12):
    raise ValueError(f'pixels of {px} bytes are unsupported: uint8 with 1, 3 or 4 channels, float32 with 1 to 3')
  if Hs * Ws * px >= 2 ** 31 or Hd * Wd * px >= 2 ** 31 or Hd > 65535 or B > 65535:
    raise ValueError(f'resize_nearest: {Hs} x {Ws} -> {Hd} x {Wd} is too large')
  t4 = t4.contiguous()
  if below is None:
    o, pitch = _out(None if out is None else _batched(out, 'out', _IMAGE_LAYOUTS)[0], (B, Hd, Wd, C), t4.dtype, dev, 'resize_nearest')
    flag = -1
  else:
    flag = int(below)
    if not 0 <= flag <= 256:
      raise ValueError(f'below={below} is outside 0..256')
    single = x.ndim < 4  # the result has no channel axis: [Hd, Wd], or [B, Hd, Wd] for a batch
    if out is not None and (not isinstance(out, torch.Tensor) or out.dim() != (2 if single else 3)):
      raise ValueError(f'resize_nearest: out must be {"[Hd, Wd]" if single else "[B, Hd, Wd]"}')
    o, pitch = _out(None if out is None else (out[None, :, :, None] if single else out[:, :, :, None]), (B, Hd, Wd, 1), torch.uint8, dev,
                    'resize_nearest')
    back = (lambda r: r[0, :, :, 0]) if single else (lambda r: r[:, :, :, 0])
  call('dyn_resize_nearest', B, Hs, Ws, px, Hd, Wd, _p(t4), _p(o), pitch, flag, stream_of(t4))
  return out if out is not None else back(o)


def erode_disk(mask, radius, out=None, device=None):
  """``skimage.morphology.erosion(mask, skimage.morphology.disk(radius))`` on a 0 / 1 mask: uint8 or bool ``[H, W]`` or ``[B, H, W]`` -> uint8 0 / 1
  of the same form.  A tap outside the image does not count (what skimage's reflect border comes to for this footprint)."""
  radius = int(radius)
  if not 0 <= radius <= MAX_RADIUS:
    raise ValueError(f'radius={radius} is outside 0..{MAX_RADIUS}')
  dev = _device(device, mask, out)
  t = _tensor(mask, 'mask', (torch.uint8, torch.bool), dev)
  if t.dtype == torch.bool:
    t = t.view(torch.uint8)
  t4, back = _batched(t, 'mask', _PLANE_LAYOUTS)
  B, H, W, _ = (int(v) for v in t4.shape)
  if H * W >= 2 ** 31 or H > 65535 or B > 65535:
    raise ValueError(f'erode_disk: {B} masks of {H} x {W} are too large (H*W < 2^31, at most 65535 rows and masks per call)')
  t4 = t4.contiguous()
  if out is not None and isinstance(out, torch.Tensor) and out.data_ptr() == t4.data_ptr():
    raise ValueError('erode_disk: out must not be the input')
  o, pitch = _out(None if out is None else _batched(out, 'out', _PLANE_LAYOUTS)[0], (B, H, W, 1), torch.uint8, dev, 'erode_disk')
  call('dyn_erode_disk_u8', B, H, W, radius, _p(t4), _p(o), pitch, stream_of(t4))
  return out if out is not None else back(o)


def depth_bounds(depth, q=(5, 95), device=None):
  """``(np.percentile(d, q[0]), np.percentile(d, q[1]))`` for each depth map (save_monocular_cameras.py:108-110): float32 ``[H, W]`` -> float32
  ``[2]`` on the device, ``[B, H, W]`` -> ``[B, 2]``; numpy's bits and dtype (a scalar ``q`` on float32 data is float32 arithmetic throughout).
  One exception: where a result is a zero its SIGN is unspecified.  The selection counts -0.0 as +0.0, as they compare, and returns +0.0 for
  either; numpy returns whichever zero its partition left at the rank (and ``-0.0 - 0.0`` where both neighbours are -0.0 and the weight is
  at least 0.5).  The values are equal, the bits may not be."""
  if len(q) != 2:
    raise ValueError(f'q must be a pair of percentiles, got {q!r}')
  dev = _device(device, depth)
  t = _tensor(depth, 'depth', (torch.float32,), dev)
  t4, _ = _batched(t, 'depth', _PLANE_LAYOUTS)
  t4 = t4.contiguous()
  B, n = int(t4.shape[0]), int(t4.shape[1]) * int(t4.shape[2])
  if n >= 2 ** 31:
    raise ValueError(f'depth maps of {n} values are too large (H*W < 2^31)')
  plans = [percentile_plan(n, v) for v in q]  # (each its own scalar call, as the script has them)
  rank = (ctypes.c_int32 * 4)(*[int(r) for p in plans for r in p[0][0]])
  weight = (ctypes.c_double * 2)(*[float(p[1][0]) for p in plans])
  out = torch.empty((B, 2), dtype=torch.float32, device=dev)
  call('dyn_percentile_pair', B, n, _p(t4), n, ctypes.cast(rank, ctypes.c_void_p), ctypes.cast(weight, ctypes.c_void_p), 1, _p(out), stream_of(t4))
  return out[0] if t.dim() == 2 else out


# ---- the loader's chains -------------------------------------------------------------------------------------------------------------
def erosion_size(size):
  """the size at which the loader erodes the motion mask of frames of ``size`` (monocular.py:184-188)"""
  w, h = _size(size)
  return int(round(288.0 * w / h)), BASE_HEIGHT


def _raw_mask(raw, what, dev):
  """a decoded mask, uint8 ``[H, W]`` or a batch ``[B, H, W]`` -> ([B, H, W, 1], how to give a result the caller's form).  A file decoded with
  colour channels, ``[H, W, 3]`` or ``[H, W, 4]``, cannot be told from a batch of narrow masks, so it is refused: pass ``m[..., 0]``, the channel
  the loader reads."""
  t = _tensor(raw, what, (torch.uint8,), dev)
  if t.dim() == 3 and t.shape[2] in (3, 4):
    raise ValueError(f'{what} is {list(t.shape)}: a mask decoded with colour channels?  Pass channel 0 ([..., 0]) as [H, W], or a batch [B, H, W]')
  if t.dim() == 2:
    return t[None, :, :, None], lambda r: r[0]
  if t.dim() == 3:
    return t[:, :, :, None], lambda r: r
  raise ValueError(f'{what} must be uint8 [H, W] or [B, H, W] as decoded (one channel), got {list(t.shape)}')


def motion_mask(raw_u8, size, radius, out=None, device=None):
  """The motion mask of monocular.py:168-203 from the decoded ``dynamic_masks`` file(s), uint8 ``[H, W]`` or ``[B, H, W]`` -> uint8 0 / 1 at
  ``size``: nearest resize to ``(round(288.0 * w / h), 288)`` of ``1 - m / 255 > 1e-3`` (``m < 255``), the disk erosion, nearest resize to
  ``size``.  (The loader's ``np.float32`` of it is the scene store's business: it holds the masks as uint8.)"""
  dev = _device(device, raw_u8, out)
  t4, back = _raw_mask(raw_u8, 'raw_u8', dev)
  small = resize_nearest(t4, erosion_size(size), below=255)         # [B, 288, w288]
  eroded = erode_disk(small, radius)
  if out is not None:
    resize_nearest(eroded[:, :, :, None], size, out=_mask_out(out, t4, 'motion_mask')[:, :, :, None])
    return out
  return back(resize_nearest(eroded[:, :, :, None], size)[:, :, :, 0])


def _mask_out(out, t4, what):
  """the caller's ``out`` ([H, W] for one mask, [B, H, W] for a batch) as [B, H, W]"""
  single = t4.shape[0] == 1 and isinstance(out, torch.Tensor) and out.dim() == 2
  if not isinstance(out, torch.Tensor) or out.dim() not in (2, 3) or (out.dim() == 2 and not single):
    raise ValueError(f'{what}: out must be a uint8 tensor [H, W] for one mask or [B, H, W] for a batch')
  return out[None] if single else out


def static_mask(raw_u8, size, out=None, device=None):
  """The static mask of monocular.py:173-181, :204 from the decoded ``static_masks`` file(s): ``np.float32(resize(1 - m / 255) > 1e-3)`` as uint8."""
  dev = _device(device, raw_u8, out)
  t4, back = _raw_mask(raw_u8, 'raw_u8', dev)
  if out is not None:
    resize_nearest(t4, size, below=255, out=_mask_out(out, t4, 'static_mask'))
    return out
  return back(resize_nearest(t4, size, below=255))


def disparity(depth, size, scale, reciprocal=True, out=None, device=None):
  """``np.load(disp_path) / scale`` (monocular.py:162) of what save_monocular_cameras.py:72, :93-95 saved: ``1.0 / depth`` in float32, the linear
  resize to ``size``, then the division by ``np.float32(scale)`` in float32 (a float32 array over a Python or numpy scalar, as the reference's
  numpy evaluates it).  ``reciprocal=False``: the input is the disparity already.  float32 ``[H, W]`` or ``[B, H, W]``."""
  divisor = float(np.float32(scale))
  if not math.isfinite(divisor) or divisor == 0.0:
    raise ValueError(f'scale={scale} is not a finite non-zero float32')
  return _linear(depth, size, out, device, reciprocal, divisor, 'disparity')


def _frames(x, what, i, j):
  """frames i..j-1 of a stack or of a list of arrays, as one array"""
  if isinstance(x, (list, tuple)):
    part = x[i:j]
    if all(isinstance(p, torch.Tensor) for p in part):
      return torch.stack(list(part))
    return np.stack([np.asarray(p) for p in part])
  return x[i:j]


def prepare_monocular(frames, depth, dynamic_masks, static_masks, flows, flow_masks, virtual_views, virtual_poses, intrinsics, poses, depth_range,
                      scale, erosion_radius, size=None, source_masks=None, batch=DEFAULT_BATCH, device=None):
  """What ``MonocularDataset`` makes of a scene's decoded files, for every frame at once and on the device -> the keyword arguments of
  ``DeviceScene``: ``DeviceScene(device, **prepare_monocular(...))``.

  frames          the decoded full-resolution frames: uint8 ``[N, Hs, Ws, 3]``, or a list of ``[Hs, Ws, 3]``
  depth           the depth maps of the ``--cvd_dir`` files (``pt_data['depth'][0, 0]``): float32 ``[N, Hd, Wd]`` or a list
  dynamic_masks, static_masks   the decoded ``dynamic_masks/%d.png`` / ``static_masks/%d.png``: uint8, one channel, ``[N, Hm, Wm]`` or lists
  flows, flow_masks, virtual_views, virtual_poses, intrinsics, poses, depth_range, source_masks   as ``DeviceScene`` takes them: these the
                  loader does not resample (monocular.py:246-266, :313)
  scale           the scene scale of ``load_mono_data``; erosion_radius  ``args.erosion_radius``
  size            ``(width, height)`` of the scene; None: ``(round(288 * Ws / Hs), 288)`` as save_monocular_cameras.py:49-51 has it
  Frames go through the kernels ``batch`` at a time, so at most that many full-resolution frames are resident; no image data returns to the
  host (``DeviceScene``'s constructor then reads back one boolean per mask store, its 0 / 1 check)."""
  dev = _device(device)
  N = len(frames)
  if min(len(depth), len(dynamic_masks), len(static_masks)) != N or max(len(depth), len(dynamic_masks), len(static_masks)) != N:
    raise ValueError(f'{N} frames, {len(depth)} depth maps, {len(dynamic_masks)} dynamic and {len(static_masks)} static masks')
  batch = int(batch)
  if batch < 1 or N < 1:
    raise ValueError(f'batch={batch}, {N} frames')
  first = np.shape(frames[0]) if not isinstance(frames[0], torch.Tensor) else tuple(frames[0].shape)
  if len(first) != 3 or first[2] != 3:
    raise ValueError(f'frames must be [N, Hs, Ws, 3], got frames of {list(first)}')
  if size is None:
    size = (int(round(BASE_HEIGHT * (float(first[1]) / float(first[0])))), BASE_HEIGHT)
  W, H = _size(size)
  images = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
  disp = torch.empty((N, H, W), dtype=torch.float32, device=dev)
  motion = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
  static = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
  for i in range(0, N, batch):
    j = min(N, i + batch)
    resize_area(_frames(frames, 'frames', i, j), (W, H), out=images[i:j], device=dev)
    disparity(_frames(depth, 'depth', i, j), (W, H), scale, out=disp[i:j], device=dev)
    motion_mask(_frames(dynamic_masks, 'dynamic_masks', i, j), (W, H), erosion_radius, out=motion[i:j], device=dev)
    static_mask(_frames(static_masks, 'static_masks', i, j), (W, H), out=static[i:j], device=dev)
  up = lambda x: x.detach().to(dev) if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
  return dict(images=images, intrinsics=intrinsics, poses=poses, depth_range=depth_range, disp=disp, motion_mask=motion, static_mask=static,
              flows=up(flows), flow_masks=up(flow_masks), virtual_views=up(virtual_views), virtual_poses=virtual_poses,
              source_masks=None if source_masks is None else up(source_masks))


# ---- virtual source views (render_source_vv.py:253-330) for every frame of a scene ------------------------------------------------------
_VV_WORKSPACE = {}    # (device, stream) -> the scratch of dyn_vv_frames, grown on demand


def _vv_workspace(F, V, H, W, dev):
  need = int(_lib.lib().dyn_vv_frames_workspace_bytes(F, V, H, W))
  if need == 0:
    raise ValueError(f'virtual views of {F} frames x {V} views of {H} x {W} are unsupported (sizes >= 1, V <= 65535, frames*views*H*W <= 2^28 per '
                     f'batch: lower batch)')
  key = (str(dev), torch.cuda.current_stream(dev).cuda_stream if dev.type == 'cuda' else 0)
  ws = _VV_WORKSPACE.get(key)
  if ws is None or ws.numel() < need:
    ws = _VV_WORKSPACE[key] = torch.empty((need,), dtype=torch.uint8, device=dev)
  return ws


def _upload(a, dev):
  """a small host float array -> float32 on ``dev`` without a synchronisation (through pinned memory, as the tables)"""
  t = torch.from_numpy(np.ascontiguousarray(a)).float().contiguous()
  return t.pin_memory().to(dev, non_blocking=True) if dev.type == 'cuda' else t


relative_transforms = vvmod.relative_transforms  # the pose algebra virtual_views.frame_batch uses


def virtual_views(images01, disp, K, c2w, vv_c2w, out=None, batch=DEFAULT_BATCH, device=None):
  """The virtual source views of N frames, ``batch`` frames x V views per ``dyn_vv_frames`` call: what
  ``np.stack([virtual_views.render_frame_virtual_views(images01[i], disp[i], K[i], c2w[i], vv_c2w[i]) for i in range(N)])`` returns, bit for
  bit, on the device and from one copy of each frame.

  images01  float32 ``[N, H, W, 3]`` in 0..1 and  disp  float32 ``[N, H, W]``, at the working size
  K         ``[3, 3]`` or ``[N, 3, 3]``: source = destination intrinsics;  c2w ``[N, 4, 4]``;  vv_c2w ``[N, V, 3, 4]`` (host arrays)
  out       None, or uint8 ``[N, V, H, W, 3]`` on the device with contiguous views at a uniform spacing (``stride(0) == V * stride(1)``)
  -> uint8 ``[N, V, H, W, 3]`` on the device.  The poses are combined on the host in float64 and K is inverted by torch on the host, both as
  the per-frame path does; nothing synchronises."""
  dev = _device(device, images01, disp, out)
  img = _tensor(images01, 'images01', (torch.float32,), dev)
  dsp = _tensor(disp, 'disp', (torch.float32,), dev)
  if img.dim() != 4 or img.shape[3] != 3 or min(img.shape) < 1:
    raise ValueError(f'images01 must be float32 [N, H, W, 3], got {list(img.shape)}')
  N, H, W, _ = (int(v) for v in img.shape)
  if tuple(dsp.shape) != (N, H, W):
    raise ValueError(f'disp must be float32 {[N, H, W]}, got {list(dsp.shape)}')
  vv = np.asarray(vv_c2w, dtype=np.float64)
  cam = np.asarray(c2w, dtype=np.float64)
  if vv.ndim != 4 or vv.shape[0] != N or vv.shape[1] < 1 or vv.shape[2:] != (3, 4) or cam.shape != (N, 4, 4):
    raise ValueError(f'c2w must be [{N}, 4, 4] and vv_c2w [{N}, V, 3, 4], got {list(cam.shape)} and {list(vv.shape)}')
  V = int(vv.shape[1])
  k = torch.from_numpy(np.array(K)).float()
  if k.dim() == 2:
    k = k[None].expand(N, 3, 3)
  if tuple(k.shape) != (N, 3, 3):
    raise ValueError(f'K must be [3, 3] or [{N}, 3, 3], got {list(k.shape)}')
  batch = int(batch)
  if batch < 1:
    raise ValueError(f'batch={batch}')
  k = k.contiguous()
  rot, tr = relative_transforms(cam, vv)
  kd, kinv, rd, td = (_upload(x, dev) for x in (k.numpy(), k.inverse().numpy(), rot.reshape(N * V, 3, 3), tr.reshape(N * V, 3)))
  if out is None:
    out = torch.empty((N, V, H, W, 3), dtype=torch.uint8, device=dev)
  else:
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != (N, V, H, W, 3):
      raise ValueError(f'virtual_views: out must be a uint8 tensor {[N, V, H, W, 3]} on {dev}')
    if not out[0, 0].is_contiguous() or (V > 1 and out.stride(1) < H * W * 3) or (N > 1 and out.stride(0) != V * out.stride(1)):
      raise ValueError('virtual_views: the views of out must be contiguous and evenly spaced (stride(0) == V * stride(1))')
  pitch = int(out.stride(1)) if V > 1 else (int(out.stride(0)) if N > 1 else H * W * 3)
  F = min(batch, N)
  ws = _vv_workspace(F, V, H, W, dev)
  for i in range(0, N, F):
    j = min(N, i + F)
    p = _lib.params('DynVvFramesParams', F=j - i, V=V, H=H, W=W, img=_p(img[i:j]), disp=_p(dsp[i:j]), k=_p(kd[i:j]), k_inv=_p(kinv[i:j]),
                    rot=_p(rd[i * V:j * V]), t=_p(td[i * V:j * V]), eps=1e-7, tenth_by_division=0 if dev.type == 'cuda' else 1, out=_p(out[i:j]),
                    out_pitch=pitch, workspace=_p(ws), workspace_bytes=int(ws.numel()))
    call('dyn_vv_frames', p, stream_of(img))
  return out


def build_virtual_views(net_images, depth, intrinsics_t, cam_c2w, size, batch=DEFAULT_BATCH, device=None, out=None):
  """render_source_vv.py from the decoded ``--cvd_dir`` records of a scene, with cv2-style resizes, on the device.

  net_images    float32 ``[N, h, w, 3]``: ``img_1`` of every record, channels last
  depth         float32 ``[N, h, w]``: ``depth[0, 0]`` of every record
  intrinsics_t  the stored transposed ``K`` of the records, ``[3, 3]`` or ``[N, 3, 3]``, for the ``w x h`` network image
  cam_c2w       ``[N, 4, 4]``;  size = ``(final_w, final_h)``
  -> (views uint8 ``[N, 8, H, W, 3]`` on the device, source_vv_poses float32 ``[8, 3, 4, N]`` on the host: the array the script saves).
  The 5th depth percentiles come from ``depth_bounds`` (one copy of N floats to the host, which the float64 pose algebra needs); the frame is
  resized with ``resize_area_f32``, ``1 / depth`` with ``resize_linear`` (reciprocal first, as the script has it)."""
  dev = _device(device, net_images, depth, out)
  img = _tensor(net_images, 'net_images', (torch.float32,), dev)
  dep = _tensor(depth, 'depth', (torch.float32,), dev)
  if img.dim() != 4 or img.shape[3] != 3 or dep.dim() != 3 or dep.shape[0] != img.shape[0] or min(img.shape) < 1 or min(dep.shape) < 1:
    raise ValueError(f'net_images must be float32 [N, h, w, 3] and depth [N, h, w], got {list(img.shape)} and {list(dep.shape)}')
  N, net_h, net_w, _ = (int(v) for v in img.shape)
  W, H = _size(size)
  Kt = np.asarray(intrinsics_t)
  Kt = np.broadcast_to(Kt, (N, 3, 3)) if Kt.ndim == 2 else Kt
  cams = [np.asarray(c) for c in cam_c2w]
  if Kt.shape != (N, 3, 3) or len(cams) != N or any(c.shape != (4, 4) for c in cams):
    raise ValueError(f'intrinsics_t must be [3, 3] or [{N}, 3, 3] and cam_c2w [{N}, 4, 4]')
  Ks = [scaled_intrinsics(Kt[i], W, H, net_w, net_h) for i in range(N)]
  fifth = depth_bounds(dep, device=dev)[:, 0].cpu().numpy()
  fx, fy = Ks[-1][0, 0], Ks[-1][1, 1]  # (the last frame's intrinsics, as in the reference)
  hwf = np.array([H, W, (fx + fy) / 2.0]).reshape([3, 1])
  vv_poses_final, vsv = vvmod.virtual_view_poses(cams, list(fifth), hwf)
  poses = np.moveaxis(vv_poses_final, 0, -1).astype(np.float32)
  V = int(vsv.shape[1])
  if out is None:
    out = torch.empty((N, V, H, W, 3), dtype=torch.uint8, device=dev)
  batch = int(batch)
  if batch < 1:
    raise ValueError(f'batch={batch}')
  for i in range(0, N, batch):
    j = min(N, i + batch)
    small = resize_area_f32(img[i:j], (W, H), device=dev)
    disp = resize_linear_reciprocal(dep[i:j], (W, H), device=dev)
    virtual_views(small, disp, np.stack(Ks[i:j]), np.stack(cams[i:j]), vsv[i:j], out=out[i:j], batch=batch, device=dev)
  return out, poses


def resize_linear_reciprocal(depth, size, out=None, device=None):
  """``cv2.resize(1.0 / depth, size, interpolation=cv2.INTER_LINEAR)``: the reciprocal in float32 first, then the resize
  (save_monocular_cameras.py:72, :93-95 and render_source_vv.py:266, :279).  float32 ``[H, W]`` or ``[B, H, W]``."""
  return _linear(depth, size, out, device, True, None, 'resize_linear_reciprocal')


# ---- the command-line tool: python -m dynibar_amd.ingest ------------------------------------------------------------------------------
def poses_bounds(c2w_mats, bounds, h, w, fx, fy):
  """The rows of ``poses_bounds_cvd.npy``, the file ``load_mono_data`` reads: ``c2w_mats`` ``[N, 4, 4]`` (or ``[N, 3, 4]``), ``bounds`` ``[N, 2]`` ->
  float64 ``[N, 17]``.  A row is a ``[3, 5]`` matrix in row-major order followed by the frame's near and far bound.  The matrix holds, per
  row of the camera-to-world rotation, its second column, its first column and its negated third column -- the camera axes (x, -y, -z) of the
  depth network re-expressed as (-y, x, z), the axis order the LLFF loaders undo -- then the translation, then one of (h, w, f) with
  ``f = (fx + fy) / 2``.  Host work."""
  c2w = np.stack([np.asarray(m) for m in c2w_mats])
  bounds = np.stack([np.asarray(b) for b in bounds])
  if c2w.ndim != 3 or c2w.shape[1] < 3 or c2w.shape[2] != 4 or bounds.shape != (c2w.shape[0], 2):
    raise ValueError(f'c2w_mats must be [N, 4, 4] and bounds [N, 2], got {list(c2w.shape)} and {list(bounds.shape)}')
  n = c2w.shape[0]
  rows = np.empty((n, 3, 5), dtype=np.float64)
  rows[:, :, 0] = c2w[:, :3, 1]
  rows[:, :, 1] = c2w[:, :3, 0]
  rows[:, :, 2] = -c2w[:, :3, 2]
  rows[:, :, 3] = c2w[:, :3, 3]
  rows[:, :, 4] = (h, w, (fx + fy) / 2.0)
  return np.concatenate([rows.reshape(n, 15), bounds.astype(np.float64)], axis=1)


def scaled_intrinsics(K, final_w, final_h, img_w, img_h):
  """The intrinsics of a depth file -- stored transposed, for the ``img_w x img_h`` image the depth network saw -- at the output size: the
  first row scales with the width, the second with the height, in the matrix's own dtype.  The pose format keeps ONE focal length, so focal
  lengths that differ by 0.5 % of their sum or more are refused."""
  K = np.array(K).T
  K = K * np.array([[final_w / img_w], [final_h / img_h], [1.0]]).astype(K.dtype)
  fx, fy = K[0, 0], K[1, 1]
  if not abs(fx - fy) < 0.005 * (fx + fy):
    raise ValueError(f'fx = {fx} and fy = {fy} differ by more than 0.5 %: the format assumes fx ~= fy')
  return K


def _decode(path):
  from PIL import Image
  return np.asarray(Image.open(path))


def _source_frame(image_dir, index):
  """the decoded full-resolution frame ``index``, with whatever channels the file has; the first frame may be a .jpg"""
  import os
  path = os.path.join(image_dir, f'{index:05d}.png')
  if index == 0 and not os.path.exists(path):
    path = os.path.join(image_dir, '00000.jpg')
  return _decode(path)


def _depth_record(path):
  """one ``--cvd_dir`` file -> (source frame index, depth float32 [h, w], transposed intrinsics [3, 3], camera-to-world [4, 4], (w, h) of the
  network's image).  The frame index is the four digits after the file name's five-letter prefix."""
  import os
  img, depth, Kt, c2w = vvmod.read_record(path)
  return int(os.path.basename(path)[5:9]), np.ascontiguousarray(depth, dtype=np.float32), Kt, c2w, (int(img.shape[1]), int(img.shape[0]))


def main(argv=None):
  """``python -m dynibar_amd.ingest --data_dir D --cvd_dir C``: what save_monocular_cameras.py leaves under ``D/dense`` -- ``images_WxH/%05d.png``,
  ``disp/%05d.npy`` (float32, not yet divided by the scene scale) and ``poses_bounds_cvd.npy`` -- from ``D/dense/images`` and the ``*.npz`` depth
  files of ``C``, with the resizes and the depth bounds on the device, ``--batch`` frames per launch."""
  import argparse
  import glob
  import os

  from PIL import Image
  ap = argparse.ArgumentParser(description='Write the resized frames, disparities and poses_bounds_cvd.npy of a monocular scene (GPU).')
  ap.add_argument('--data_dir', required=True, help='the scene: frames are read from <data_dir>/dense/images, results go under <data_dir>/dense')
  ap.add_argument('--cvd_dir', required=True, help='the folder with the consistent-depth results, one .npz per frame')
  ap.add_argument('--batch', type=int, default=DEFAULT_BATCH, help='frames per kernel launch')
  ap.add_argument('--virtual_views', action='store_true',
                  help='also write source_virtual_views_WxH/NNNNN/KK.png and source_vv_poses.npy (render_source_vv.py) with cv2-style resizes')
  a = ap.parse_args(argv)
  records = sorted(glob.glob(os.path.join(a.cvd_dir, '*.npz')))
  if not records:
    raise SystemExit(f'no *.npz under {a.cvd_dir}')
  if a.batch < 1:
    raise SystemExit('--batch must be at least 1')
  dense = os.path.join(a.data_dir, 'dense')
  image_dir = os.path.join(dense, 'images')
  src_h, src_w = _source_frame(image_dir, 0).shape[:2]
  out_h = BASE_HEIGHT
  out_w = int(round(out_h * (float(src_w) / float(src_h))))
  frame_out, disp_out = os.path.join(dense, f'images_{out_w}x{out_h}'), os.path.join(dense, 'disp')
  for d in (frame_out, disp_out):
    os.makedirs(d, exist_ok=True)
  dev = _device(None)
  cams, bounds, K = [], [], None
  for start in range(0, len(records), a.batch):
    chunk = [_depth_record(p) for p in records[start:start + a.batch]]
    for _, _, Kt, c2w, (net_w, net_h) in chunk:
      K = scaled_intrinsics(Kt, out_w, out_h, net_w, net_h)
      cams.append(c2w)
    depth = torch.from_numpy(np.stack([r[1] for r in chunk])).to(dev)
    frames = np.stack([_source_frame(image_dir, r[0]) for r in chunk])
    small = resize_area(frames, (out_w, out_h), device=dev).cpu().numpy()
    disp = disparity(depth, (out_w, out_h), 1.0, device=dev).cpu().numpy()
    bounds.extend(depth_bounds(depth).cpu().numpy())
    for k in range(len(chunk)):
      Image.fromarray(small[k]).save(os.path.join(frame_out, f'{start + k:05d}.png'))
      np.save(os.path.join(disp_out, f'{start + k:05d}.npy'), disp[k])
  np.save(os.path.join(dense, 'poses_bounds_cvd.npy'), poses_bounds(cams, bounds, out_h, out_w, K[0, 0], K[1, 1]))
  if a.virtual_views:
    write_virtual_views(records, dense, (out_w, out_h), a.batch, dev)
  return 0


def write_virtual_views(records, dense, size, batch=DEFAULT_BATCH, device=None):
  """The files of render_source_vv.py from the ``*.npz`` depth records, under ``dense``: ``source_virtual_views_WxH/NNNNN/KK.png`` and
  ``source_vv_poses.npy`` -> the list of the PNG paths, in the order ``virtual_views.main`` reports them."""
  import os
  net, depth, Kt, cams = zip(*(vvmod.read_record(path) for path in records))
  f32 = lambda xs: np.stack([np.ascontiguousarray(x, dtype=np.float32) for x in xs])
  views, poses = build_virtual_views(f32(net), f32(depth), np.stack(Kt), list(cams), size, batch=batch, device=device)
  np.save(os.path.join(dense, 'source_vv_poses.npy'), poses)
  save_dir = os.path.join(dense, 'source_virtual_views_%dx%d' % size)
  written = []
  for i in range(len(records)):
    written += vvmod.write_frame_views(save_dir, i, views[i].cpu().numpy())
  return written


if __name__ == '__main__':
  raise SystemExit(main())
