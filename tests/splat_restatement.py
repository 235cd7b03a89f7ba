"""Yardstick of the virtual-source-view kernels (dynibar_amd/csrc/dyn_splat.h): numpy restatements, no torch, no device.

* ``splat_f32``: the summation splat of the ``splatting`` package (the package is not installed here; its published definition is the
  contract, include/dynibar_hip.h).  Source pixel (x, y) goes to X = x + flow_x, Y = y + flow_y (fp32), corners nw, ne, sw, se of
  (floor X, floor Y) get w * value, w = products of (x0 + 1 - X), (X - x0), (y0 + 1 - Y), (Y - y0); off-image corners and targets outside
  [-1, W) x [-1, H) (NaN, inf included) contribute nothing.  Every destination is summed in float32, one contribution at a time, in
  ascending contribution id 4 (y W + x) + corner, from +0.0: ``np.add.at`` applies its updates sequentially in the order given.
  The GPU and emulator results must equal this BITWISE.
* ``project_f64`` / ``sobel_alpha_f64``: the projection of render_source_vv.py:15-53 and the Sobel alpha of :118-128 in float64.
* ``finish_u8``: the epilogue of :313-330 in float32 numpy as the script does it, the erosion by scipy.ndimage.
"""
import numpy as np


def _taps(flow_b, H, W):
  """-> per source pixel (row-major) and corner: target index (or -1), weight; both [H*W, 4] in contribution-id order."""
  f32 = np.float32
  yy, xx = np.mgrid[0:H, 0:W]
  with np.errstate(invalid='ignore', over='ignore'):
    X = xx.astype(f32) + flow_b[0].astype(f32)
    Y = yy.astype(f32) + flow_b[1].astype(f32)
    ok = (X >= f32(-1)) & (X < f32(W)) & (Y >= f32(-1)) & (Y < f32(H))
  X = np.where(ok, X, f32(0)).reshape(-1)
  Y = np.where(ok, Y, f32(0)).reshape(-1)
  ok = ok.reshape(-1)
  x0, y0 = np.floor(X), np.floor(Y)
  ax, bx = (x0 + f32(1)) - X, X - x0
  ay, by = (y0 + f32(1)) - Y, Y - y0
  w = np.stack([ax * ay, bx * ay, ax * by, bx * by], 1)
  xi, yi = x0.astype(np.int64), y0.astype(np.int64)
  cx = np.stack([xi, xi + 1, xi, xi + 1], 1)
  cy = np.stack([yi, yi, yi + 1, yi + 1], 1)
  inside = ok[:, None] & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
  tgt = np.where(inside, cy * W + cx, -1)
  return tgt, w.astype(f32)


def splat_f32(frame, flow, mult=None, normalize=False, eps=1e-7):
  """frame [B,C,H,W], flow [B,2,H,W], mult [B,H,W] or None -> [B,C,H,W] float32 (see the module docstring)."""
  frame = np.asarray(frame, np.float32)
  flow = np.asarray(flow, np.float32)
  B, C, H, W = frame.shape
  out = np.zeros((B, C, H * W), np.float32)
  den = np.zeros((B, H * W), np.float32)
  for b in range(B):
    tgt, w = _taps(flow[b], H, W)
    tgt, w = tgt.reshape(-1), w.reshape(-1)
    keep = tgt >= 0
    src = np.repeat(np.arange(H * W), 4)[keep]
    t, wk = tgt[keep], w[keep]
    m = np.ones(H * W, np.float32) if mult is None else np.asarray(mult, np.float32)[b].reshape(-1)
    for c in range(C):
      f = frame[b, c].reshape(-1)
      if mult is not None:
        f = f * m
      with np.errstate(invalid='ignore', over='ignore'):
        np.add.at(out[b, c], t, wk * f[src])
    if normalize:
      np.add.at(den[b], t, wk * m[src])
  if normalize:
    with np.errstate(divide='ignore', invalid='ignore'):
      out = out / (den[:, None] + np.float32(eps))
  return out.reshape(B, C, H, W)


def forward_splat_f32(src, flow, importance, weight_exp, eps=1e-7):
  """The softmax splat of render_forward_splat on given flow / importance / exp(w) (the kernel's probe outputs): src [B,H,W,C] ->
  (feat [B,C,H,W], disp [B,1,H,W], mask [B,1,H,W])."""
  src = np.asarray(src, np.float32)
  B, H, W, C = src.shape
  frame = np.concatenate([src.transpose(0, 3, 1, 2), np.asarray(importance, np.float32)[:, None], np.ones((B, 1, H, W), np.float32)], 1)
  out = splat_f32(frame, flow, weight_exp, normalize=True, eps=eps)
  return out[:, :C], out[:, C:C + 1], out[:, C + 1:C + 2]


def project_f64(depth, k_src_inv, rot, t, k_dst):
  """float64 flow [B,2,H,W], importance [B,H,W], exp(w) [B,H,W] of render_source_vv.py:23-53."""
  depth = np.asarray(depth, np.float64)
  B, H, W = depth.shape
  yy, xx = np.mgrid[0:H, 0:W]
  coord = np.stack([xx, yy, np.ones_like(xx)], -1).astype(np.float64)  # [H,W,3]
  P = depth[..., None] * np.einsum('bij,hwj->bhwi', np.asarray(k_src_inv, np.float64), coord)
  S = np.einsum('bij,bhwj->bhwi', np.asarray(rot, np.float64), P) + np.asarray(t, np.float64)[:, None, None, :]
  Q = np.einsum('bij,bhwj->bhwi', np.asarray(k_dst, np.float64), S)
  z = Q[..., 2]
  zc = np.maximum(z, 1e-8)
  flow = np.stack([Q[..., 0] / zc - xx, Q[..., 1] / zc - yy], 1)
  imp = 1.0 / z
  lo = imp.min(axis=(1, 2), keepdims=True)
  hi = imp.max(axis=(1, 2), keepdims=True)
  w = (imp - lo) / (hi - lo + 1e-6) * 20 - 10
  return flow, imp, np.exp(w)


def sobel_alpha_f64(x, beta):
  """x [B,1,H,W] -> exp(-beta |(gx, gy)|), Sobel cross-correlation with replicate padding, in float64."""
  x = np.asarray(x, np.float64)
  p = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode='edge')
  kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.float64)
  H, W = x.shape[2:]
  gx = np.zeros_like(x)
  gy = np.zeros_like(x)
  for i in range(3):
    for j in range(3):
      win = p[:, :, i:i + H, j:j + W]
      gx += kx[i, j] * win
      gy += kx.T[i, j] * win
  return np.exp(-beta * np.sqrt(gx * gx + gy * gy))


def erode_disk1(mask):
  """skimage.morphology.erosion(mask, disk(1)) for a boolean [H,W]: grey erosion with the 3x3 cross, mode 'reflect'."""
  import scipy.ndimage as ndi
  disk1 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
  return ndi.grey_erosion(mask.astype(np.uint8), footprint=disk1, mode='reflect').astype(bool)


def finish_u8(feat):
  """feat [B,C>=4,H,W] float32 -> uint8 [B,H,W,3] exactly as render_source_vv.py:313-330 forms each view's PNG."""
  feat = np.asarray(feat, np.float32)
  outs = []
  for f in feat:
    rgb = np.clip(f[:3].transpose(1, 2, 0) / 255.0, 0.0, 1.0)
    mask = np.clip(f[3:4].transpose(1, 2, 0), 0.0, 1.0)
    mask = erode_disk1(mask[..., 0] > 0.5)
    outs.append(np.uint8(255 * np.clip(rgb * mask[..., None], 0.0, 1.0)))
  return np.stack(outs)
