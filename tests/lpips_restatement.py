"""Yardstick of the LPIPS kernels (dynibar_amd/csrc/dyn_lpips.h): the contract of DESIGN.md section 4.19 restated in torch on the CPU, once in
float64 (the oracle) and once in float32 (the reference's arithmetic).  No device, nothing of the package under test.

* ``prepare_scaled``: eval_nvidia.py:383-396, ``im2tensor`` (:250-263) and the scaling layer in float32 numpy.  The device must equal it BITWISE.
* ``features(x, weights, dtype)``: torchvision's AlexNet ``features`` with ``F.conv2d`` / ``F.max_pool2d``, tapped after each ReLU.
* ``maps(...)``: ``d_l = sum_c lin_l[c] (n0 - n1)^2``, ``n = f / (sqrt(sum_c f^2) + 1e-10)``.
* ``resize_mask`` / ``nearest_index``: the integer nearest rule ``src = (dst * n_in) // n_out``.
* ``masked_lpips``: ``sum_l (sum d_l m_l) / (sum m_l)``, a tap with an empty mask contributing 0.
* ``random_weights(seed)``: convolution weights normal * sqrt(2 / fan_in), bias normal * 0.1, lin uniform in [0, 0.1), as the two state dicts
  ``LPIPS(...)`` takes.  ``make_pair``: the image pairs of the tests.

NOT a check against the script's ``models`` package (NSFF's modified LPIPS): that package and the pretrained weights were not available.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SHAPES = ((31, 31), (32, 45), (67, 95), (288, 512))
PAIRS = ('noisy', 'close', 'border')
CHANNELS = (64, 192, 384, 256, 256)
FEATURE_INDEX = (0, 3, 6, 8, 10)
CONV = ((64, 3, 11, 4, 2), (192, 64, 5, 1, 2), (384, 192, 3, 1, 1), (256, 384, 3, 1, 1), (256, 256, 3, 1, 1))  # cout, cin, k, stride, pad
SHIFT = np.array([-.030, -.088, -.188], np.float32)
SCALE = np.array([.458, .448, .450], np.float32)


def tap_sizes(H, W):
  c1 = lambda n: (n + 4 - 11) // 4 + 1
  pool = lambda n: (n - 3) // 2 + 1
  s1 = (c1(H), c1(W))
  s2 = (pool(s1[0]), pool(s1[1]))
  s3 = (pool(s2[0]), pool(s2[1]))
  return (s1, s2, s3, s3, s3)


@functools.lru_cache(maxsize=4)
def random_weights(seed):
  """-> (alexnet_state_dict, lin_state_dict) of float32 tensors with torchvision's and the lpips package's keys"""
  g = torch.Generator().manual_seed(1000 + seed)
  alex, lin = {}, {}
  for i, (co, ci, k, _, _) in zip(FEATURE_INDEX, CONV):
    alex[f'features.{i}.weight'] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
    alex[f'features.{i}.bias'] = torch.randn(co, generator=g) * 0.1
  for l, c in enumerate(CHANNELS):
    lin[f'lin{l}.model.1.weight'] = torch.rand(1, c, 1, 1, generator=g) * 0.1
  return alex, lin


@functools.lru_cache(maxsize=32)
def make_pair(H, W, kind, seed=0):
  """-> pred float32 [H, W, 3] in [0, 1], target uint8 [H, W, 3].  noisy: clip(a + 0.1 n); close: + 0.005 n; border: a prediction with a black
  border and black blobs, so that the valid mask bites."""
  rng = np.random.RandomState(7919 * seed + 13 * H + W + PAIRS.index(kind))
  yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
  base = np.stack([0.5 + 0.4 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0 - c) for c in range(3)], -1).astype(np.float32)
  base = np.clip(base + 0.2 * rng.rand(H, W, 3).astype(np.float32) - 0.1, 0, 1)
  target = np.round(base * 255).astype(np.uint8)
  a = target.astype(np.float32) / np.float32(255)
  sigma = 0.005 if kind == 'close' else 0.1
  pred = np.clip(a + np.float32(sigma) * rng.randn(H, W, 3).astype(np.float32), 0, 1).astype(np.float32)
  if kind == 'border':
    pred[:3] = 0
    pred[:, -4:] = 0
    for _ in range(3):
      y, x = rng.randint(0, H - 6), rng.randint(0, W - 6)
      pred[y:y + 6, x:x + 5] = 0
  return pred, target


def prepare_scaled(pred, target, apply_valid=True):
  """-> (x0, x1) float32 [H, W, 3]: the prepared images through im2tensor and the scaling layer, and valid [H, W] float32"""
  valid = np.float32(np.sum(pred, axis=-1, keepdims=True) > 1e-3)
  if target.dtype == np.uint8:
    target = np.float32(target) / 255
  a, b = (pred * valid, target * valid) if apply_valid else (pred, target)
  out = []
  for x in (a, b):
    t = x / np.float32(0.5) - np.float32(1.0)
    out.append(((t - SHIFT) / SCALE).astype(np.float32))
  assert out[0].dtype == np.float32
  return out[0], out[1], valid[..., 0]


def features(x, alex, dtype):
  """x [N, 3, H, W] -> the five taps [N, C_l, H_l, W_l]"""
  taps = []
  for n, (i, (_, _, _, stride, pad)) in enumerate(zip(FEATURE_INDEX, CONV)):
    if n in (1, 2):
      x = F.max_pool2d(x, 3, 2)
    x = F.relu(F.conv2d(x, alex[f'features.{i}.weight'].to(dtype), alex[f'features.{i}.bias'].to(dtype), stride=stride, padding=pad))
    taps.append(x)
  return taps


def maps(x0, x1, weights, dtype):
  """the scaled images [H, W, 3] float32 -> the five d_l [H_l, W_l] in ``dtype``"""
  alex, lin = weights
  x = torch.from_numpy(np.stack([x0, x1])).permute(0, 3, 1, 2).to(dtype)
  out = []
  with torch.no_grad():
    for l, f in enumerate(features(x, alex, dtype)):
      n = f / (torch.sqrt(torch.sum(f * f, dim=1, keepdim=True)) + 1e-10)
      w = lin[f'lin{l}.model.1.weight'].to(dtype)
      out.append(torch.sum(w * (n[0:1] - n[1:2]) ** 2, dim=1)[0].numpy())
  return out


def nearest_index(n_out, n_in):
  return (np.arange(n_out, dtype=np.int64) * n_in) // n_out


def resize_mask(mask, h, w):
  """channel 0 of a [H, W], [H, W, 1] or [H, W, 3] mask at the tap's resolution, as float64"""
  m = mask if mask.ndim == 2 else mask[..., 0]
  return m[nearest_index(h, m.shape[0])][:, nearest_index(w, m.shape[1])].astype(np.float64)


def masked_sums(ds, mask):
  """-> [(S_l, M_l)] in longdouble"""
  out = []
  for d in ds:
    m = resize_mask(mask, *d.shape).astype(np.longdouble)
    out.append(((d.astype(np.longdouble) * m).sum(), m.sum()))
  return out


def masked_lpips(ds, mask):
  return float(sum((s / m if m != 0 else 0) for s, m in masked_sums(ds, mask)))


def make_masks(H, W, seed=0):
  """six masks [H, W, 1] float32: ones, a dynamic 0 / 1 blob, its complement, fractional weights (multiples of 1 / 256: their sums are exact in
  double in any order), a mask that is zero at one whole tap's resolution (it is nonzero only where the last taps' nearest rule never looks,
  so taps 3-5 see an empty mask and taps 1-2 do not), all zeros"""
  rng = np.random.RandomState(31 * seed + H + W)
  yy, xx = np.mgrid[0:H, 0:W]
  dyn = (((yy - H * 0.4) / (H * 0.3)) ** 2 + ((xx - W * 0.55) / (W * 0.25)) ** 2 < 1).astype(np.float32)
  frac = (rng.randint(0, 257, size=(H, W)) / 256.0).astype(np.float32)
  sizes = tap_sizes(H, W)
  looked = np.zeros((H, W), bool)
  looked[np.ix_(nearest_index(sizes[4][0], H), nearest_index(sizes[4][1], W))] = True
  gap = (~looked).astype(np.float32)
  ms = dict(ones=np.ones((H, W), np.float32), dynamic=dyn, static=1 - dyn, fractional=frac, gap=gap, zero=np.zeros((H, W), np.float32))
  return {k: v[..., None] for k, v in ms.items()}


MASKS = ('ones', 'dynamic', 'static', 'fractional', 'gap', 'zero')
