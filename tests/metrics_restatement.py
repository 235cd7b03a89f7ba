"""Yardstick of the frame-metrics kernels (dynibar_amd/csrc/dyn_metrics.h): numpy / scipy restatements, no torch, no device.

* ``prepare``: eval_nvidia.py:383-396 as the script writes it, in float32 numpy.  The device must equal it BITWISE.
* ``ssim_map_uniform(a, b, R, dtype)``: the algorithm of ``skimage.metrics.structural_similarity`` as the script calls it (:242-244: defaults,
  channel axis last, ``full=True``) with ``scipy.ndimage.uniform_filter`` -- (A) in float64 (what skimage computes after casting to float64),
  (B) in float32.  skimage itself is not installed where this was written: this is a restatement of its published algorithm, not its output.
* ``ssim_map_exact`` (E): the same formulas with direct 49-term window sums over a ``symmetric``-padded array in ``np.longdouble``.  The module
  asserts that longdouble is the 80-bit x87 format (eps < 1e-18); where it is not, importing fails and the tests fail, not skip.
* ``psnr_reference`` / ``ssim_reference``: the last lines of the script's calculate_psnr / calculate_ssim (:214-225, :245-247).
* ``make_case``: seeded images built like a render, and the masks (see its docstring).
"""
import functools
import math

import numpy as np
from scipy.ndimage import uniform_filter

assert np.finfo(np.longdouble).eps < 1e-18, 'np.longdouble is not the 80-bit extended format here: the exact form (E) has no head room over float64'

PREDICTIONS = ('noisy', 'close', 'flatdark', 'bright', 'identical')
MASKS = ('ones', 'valid', 'dynamic', 'static', 'zero', 'fractional')
EPS53 = 2.0 ** -53


def c1c2(R, dt=np.float64):
  return (dt(0.01) * dt(R)) ** 2, (dt(0.03) * dt(R)) ** 2


def map_limit(R):
  """B(R) = 144 * 2^-53 / C2(R): the only ill-conditioned step is uxx - ux^2 (and its two siblings), a difference of values <= 1 each within
  48 * 2^-53 of exact (49-term double sums of exact products), three such terms per variance, over a denominator >= C2."""
  return 144 * EPS53 / float(c1c2(R)[1])


def prepare(pred, target):
  """(:383-396) -> prepared pred, prepared target, valid [H,W,3] float32"""
  valid = np.float32(np.sum(pred, axis=-1, keepdims=True) > 1e-3)
  valid = np.tile(valid, (1, 1, 3))
  if target.dtype == np.uint8:
    target = np.float32(target) / 255
  return pred * valid, target * valid, valid


def _ssim_from_means(ux, uy, uxx, uyy, uxy, R, dt):
  cn = dt(49) / dt(48)
  C1, C2 = c1c2(R, dt)
  vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
  return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim_map_uniform(a, b, R, dtype=np.float64):
  """(A) dtype=float64, (B) dtype=float32: uniform_filter(size=7), scipy's default `reflect` boundary, per channel; not cropped"""
  a, b = a.astype(dtype), b.astype(dtype)
  S = np.empty(a.shape, dtype)
  for c in range(a.shape[2]):
    x, y = a[..., c], b[..., c]
    S[..., c] = _ssim_from_means(*(uniform_filter(q, size=7) for q in (x, y, x * x, y * y, x * y)), R, dtype)
  return S


def _box_exact(x):
  p = np.pad(x, 3, mode='symmetric')  # numpy's `symmetric` is scipy's `reflect`: d c b a | a b c d
  H, W = x.shape
  out = np.zeros((H, W), np.longdouble)
  for dy in range(7):
    for dx in range(7):
      out += p[dy:dy + H, dx:dx + W]
  return out / np.longdouble(49)


def exact_means(a, b):
  """the five window means per channel in longdouble (the slow part of (E); independent of R)"""
  a, b = a.astype(np.longdouble), b.astype(np.longdouble)
  return [[_box_exact(q) for q in (a[..., c], b[..., c], a[..., c] * a[..., c], b[..., c] * b[..., c], a[..., c] * b[..., c])]
          for c in range(a.shape[2])]


def ssim_map_exact(a, b, R, means=None):
  """(E) -> longdouble [H,W,3]"""
  means = exact_means(a, b) if means is None else means
  return np.stack([_ssim_from_means(*m, R, np.longdouble) for m in means], -1)


def masked_sums_exact(a, b, S, mask):
  """sum((a - b)^2 m), sum(S m), sum(m) in longdouble; mask [H,W,3] or [H,W,1]"""
  L = np.longdouble
  m = np.broadcast_to(mask, a.shape).astype(L)
  d = a.astype(L) - b.astype(L)
  return np.sum(d * d * m), np.sum(S.astype(L) * m), np.sum(m)


def psnr_reference(sse, msum):
  num_valid = float(msum) + 1e-8
  mse = float(sse) / num_valid
  if mse == 0:
    return 0
  return 10 * math.log10(1.0 / mse)


def ssim_reference(ssum, msum):
  return float(ssum) / (float(msum) + 1e-8)


def calculate_psnr_restated(img1, img2, mask):
  """calculate_psnr (:201-225) line by line"""
  img1 = img1.astype(np.float64)
  img2 = img2.astype(np.float64)
  mask = mask.astype(np.float64)
  num_valid = np.sum(mask) + 1e-8
  mse = np.sum((img1 - img2) ** 2 * mask) / num_valid
  if mse == 0:
    return 0
  return 10 * math.log10(1.0 / mse)


def threshold_band(n, rng):
  """n pixels [n,3] float32 around the valid threshold: channel sum exactly float32(1e-3) (NOT valid), one ulp below, one ulp above, and
  triples whose decision depends on the order of the three additions ((r + g) + b against r + (g + b))"""
  f32 = np.float32
  t = f32(1e-3)
  r = (rng.random(4096, dtype=np.float32) * (t / f32(2))).astype(f32)
  g = (rng.random(4096, dtype=np.float32) * (t / f32(2))).astype(f32)
  b = (t - (r + g)).astype(f32)
  b = np.where(rng.random(4096) < 0.5, b, np.nextafter(b, f32(1)))
  s1, s2 = (r + g) + b, r + (g + b)
  odd = np.nonzero((s1 > t) != (s2 > t))[0]
  assert odd.size >= 8, 'the generator found too few order-dependent triples'
  out = np.zeros((n, 3), f32)
  for i in range(n):
    k = i % 4
    if k == 0:
      out[i] = (t, 0, 0)
    elif k == 1:
      out[i] = (np.nextafter(t, f32(0)), 0, 0)
    elif k == 2:
      out[i] = (0, np.nextafter(t, f32(1)), 0)
    else:
      j = odd[(i // 4) % odd.size]
      out[i] = (r[j], g[j], b[j])
  return out


@functools.lru_cache(maxsize=4)
def make_case(H, W, name, seed=0):
  """-> dict: pred float32 [H,W,3], target_u8 uint8 [H,W,3], target float32 (= float32(u8) / 255), masks {name: float32 [H,W,3]}.

  The target is smooth and quantised to 1/255 like a decoded image; the prediction is `noisy` (sigma 0.05), `close` (sigma 0.002), `flatdark`
  (0.02 +- 1e-4 against a constant), `bright` (0.98 +- 1e-3 against a constant: the worst conditioning of uxx - ux^2) or `identical`.  Every
  prediction has a blanked rectangle of exact zeros (pixels the renderer did not cover) and, in row H // 2, the band of `threshold_band`."""
  assert name in PREDICTIONS
  rng = np.random.default_rng([seed, H, W, PREDICTIONS.index(name)])
  yy, xx = np.mgrid[0:H, 0:W]
  if name == 'flatdark':
    u8 = np.full((H, W, 3), 5, np.uint8)
  elif name == 'bright':
    u8 = np.full((H, W, 3), 250, np.uint8)
  else:
    u8 = np.stack([np.round((0.5 + 0.4 * np.sin(xx / 17 + c) * np.cos(yy / 11)) * 255) for c in range(3)], -1).astype(np.uint8)
  target = np.float32(u8) / 255
  sigma = dict(noisy=0.05, close=0.002, flatdark=1e-4, bright=1e-3, identical=0.0)[name]
  pred = target.copy()
  if sigma:
    pred = np.clip(target + rng.normal(0, sigma, target.shape), 0, 1).astype(np.float32)
  pred[:max(1, H // 7), :max(1, W // 8)] = 0
  pred[H // 2] = threshold_band(W, rng)
  if name == 'identical':  # the same bits on both sides after the preparation: the band's target follows the prediction where it stays valid
    target = pred.copy()
    u8 = None
  valid = prepare(pred, target)[2]
  blob = (((yy - 0.45 * H) / (0.3 * H)) ** 2 + ((xx - 0.55 * W) / (0.25 * W)) ** 2 < 1).astype(np.float32)
  dynamic = np.tile(blob[..., None], (1, 1, 3))
  masks = dict(ones=np.ones((H, W, 3), np.float32), valid=valid, dynamic=dynamic, static=1 - dynamic, zero=np.zeros((H, W, 3), np.float32),
               fractional=rng.random((H, W, 3), dtype=np.float32))
  return dict(pred=pred, target=target, target_u8=u8, masks=masks)
