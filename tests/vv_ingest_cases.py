"""Support for the tests of the float INTER_AREA (dyn_resize_area_f32) and of the batched virtual views (dyn_vv_frames, ingest.virtual_views,
ingest.build_virtual_views): a numpy restatement of the resize contract in include/dynibar_hip.h, its float64 evaluation, seeded inputs and the
checks the device and the emulator tests share.  Test infrastructure: nothing in dynibar_amd imports this.

The yardstick of the batched views is the per-frame path that existed before them, virtual_views.render_frame_virtual_views: every comparison
with it is exact."""
import functools

import numpy as np
import torch

import ingest_cases as ic

F32 = np.float32
ENLARGE = (9, 13, 16, 23)   # Hs, Ws, Hd, Wd: both axes enlarge
MIXED = (20, 9, 8, 23)      # rows shrink, columns enlarge
AREA_F32_CASES = list(ic.AREA_SHAPES) + [ENLARGE, MIXED]
VV_SHAPE = (3, 8, 24, 40)   # F, V, H, W


# ---- the float INTER_AREA ------------------------------------------------------------------------------------------------------------
def f01_image(*shape, seed=0):
  return np.random.default_rng([seed, 31] + list(shape)).random(shape, dtype=np.float32)


def area_branch(Hs, Ws, Hd, Wd):
  if Hd > Hs or Wd > Ws:
    return 'enlarge'
  return 'block' if ic.area_is_integer(Hs, Ws, Hd, Wd) else 'table'


def enlarge_axis(s, d):
  """-> (first tap int64 [d], weight of the second tap float32 [d])"""
  inv = float(d) / s
  scale = 1.0 / inv
  i = np.arange(d, dtype=np.float64)
  s0 = np.floor(i * scale)
  f = ((i + 1) - (s0 + 1) * inv).astype(F32)
  f = np.where(f <= 0, F32(0), f - np.floor(f)).astype(F32)
  return s0.astype(np.int64), f


def _block_taps(src, Hd, Wd, ix, iy):
  return [src[q::iy][:Hd][:, p::ix][:, :Wd] for q in range(iy) for p in range(ix)]  # k = q * ix + p


def resize_area_f32(src, size, dtype=F32):
  """dyn_resize_area_f32 for one image, float32 [H, W, C], size = (width, height).  dtype=np.float64: the same weighted average with the same
  fp32 coefficients promoted to double and every operation in double."""
  Hs, Ws, C = src.shape
  Wd, Hd = size
  S = src.astype(dtype)
  branch = area_branch(Hs, Ws, Hd, Wd)
  if branch == 'block':
    ix, iy = int(ic.axis_scale(Ws, Wd)), int(ic.axis_scale(Hs, Hd))
    if ix * iy == 1:
      return S.copy()
    taps = _block_taps(S, Hd, Wd, ix, iy)
    total = np.zeros((Hd, Wd, C), dtype)
    k = 0
    while k <= len(taps) - 4:
      total = total + (((taps[k] + taps[k + 1]) + taps[k + 2]) + taps[k + 3])
      k += 4
    for t in taps[k:]:
      total = total + t
    return total * dtype(F32(1) / F32(ix * iy))
  if branch == 'table':
    xt, yt = ic.decimation_table(Ws, Wd), ic.decimation_table(Hs, Hd)
    rows = np.zeros((Hs, Wd, C), dtype)
    for dx, row in enumerate(xt):
      acc = np.zeros((Hs, C), dtype)
      for k, a in row:
        acc = acc + S[:, k, :] * dtype(a)
      rows[:, dx, :] = acc
    out = np.zeros((Hd, Wd, C), dtype)
    for dy, row in enumerate(yt):
      acc = None
      for k, b in row:
        t = dtype(b) * rows[k]
        acc = t if acc is None else acc + t
      out[dy] = acc
    return out
  sx, fx = enlarge_axis(Ws, Wd)
  edge = sx >= Ws - 1
  a = np.minimum(sx, Ws - 1)
  b = np.minimum(a + 1, Ws - 1)
  wx1 = fx.astype(dtype)[None, :, None]
  wx0 = (F32(1) - fx).astype(dtype)[None, :, None]
  rows = np.where(edge[None, :, None], S[:, a], S[:, a] * wx0 + S[:, b] * wx1).astype(dtype)
  sy, fy = enlarge_axis(Hs, Hd)
  r0, r1 = np.clip(sy, 0, Hs - 1), np.clip(sy + 1, 0, Hs - 1)
  wy1 = fy.astype(dtype)[:, None, None]
  wy0 = (F32(1) - fy).astype(dtype)[:, None, None]
  return (rows[r0] * wy0 + rows[r1] * wy1).astype(dtype)


def area_taps(Hs, Ws, Hd, Wd):
  """the number of taps of every destination row and column -> (n_y int [Hd], n_x int [Wd])"""
  branch = area_branch(Hs, Ws, Hd, Wd)
  if branch == 'block':
    return np.full(Hd, int(ic.axis_scale(Hs, Hd))), np.full(Wd, int(ic.axis_scale(Ws, Wd)))
  if branch == 'table':
    return np.array([len(r) for r in ic.decimation_table(Hs, Hd)]), np.array([len(r) for r in ic.decimation_table(Ws, Wd)])
  return np.full(Hd, 2), np.full(Wd, 2)


def _bits(a):
  return np.ascontiguousarray(a, F32).view(np.uint32)


def check_area_f32(dev, Hs, Ws, Hd, Wd, C, seed=0):
  from dynibar_amd import ingest
  src = f01_image(Hs, Ws, C, seed=seed)
  want = resize_area_f32(src, (Wd, Hd))
  d = ic.dev_t(src, dev)
  ingest.resize_area_f32(d, (Wd, Hd))  # (the first call of a size uploads its tables)
  with ic.no_sync(dev):
    got = ingest.resize_area_f32(d, (Wd, Hd))
    again = ingest.resize_area_f32(d, (Wd, Hd))
  assert got.dtype == torch.float32 and tuple(got.shape) == (Hd, Wd, C)
  g = ic.host(got)
  assert np.array_equal(_bits(g), _bits(want)), f'{int(np.sum(_bits(g) != _bits(want)))} values differ, max {np.abs(g - want).max():.3e}'
  assert torch.equal(got, again)
  if (Hs, Ws) == (Hd, Wd):  # the 1 x 1 scale is the identity
    assert np.array_equal(_bits(g), _bits(src))
  if C == 1:  # the [H, W] form and a host array
    assert np.array_equal(_bits(ic.host(ingest.resize_area_f32(src[:, :, 0], (Wd, Hd), device=dev))), _bits(want[:, :, 0]))


def check_area_f32_pitched(dev, Hs=15, Ws=23, Hd=4, Wd=6, C=3, B=2, pad=5):
  """B images into a store whose rows are longer than an image: the padding keeps its bytes"""
  from dynibar_amd import ingest
  src = f01_image(B, Hs, Ws, C, seed=3)
  n = Hd * Wd * C
  store = torch.full((B, n + pad), -7.5, dtype=torch.float32, device=dev)
  view = store[:, :n].view(B, Hd, Wd, C)
  ret = ingest.resize_area_f32(ic.dev_t(src, dev), (Wd, Hd), out=view)
  assert ret is view
  got = ic.host(store)
  for b in range(B):
    assert np.array_equal(_bits(got[b, :n].reshape(Hd, Wd, C)), _bits(resize_area_f32(src[b], (Wd, Hd)))), b
  assert np.array_equal(_bits(got[:, n:]), _bits(np.full((B, pad), -7.5, F32))), 'the padding was written'


def check_area_f32_refusals(dev):
  import pytest
  from dynibar_amd import ingest
  with pytest.raises(ValueError, match='1 to 4 channels'):
    ingest.resize_area_f32(ic.dev_t(f01_image(6, 8, 5), dev), (4, 3))
  wide = ic.dev_t(f01_image(6, 16, 3), dev)
  with pytest.raises(ValueError, match='contiguous'):
    ingest.resize_area_f32(wide[:, ::2], (4, 3))
  d = ic.dev_t(f01_image(6, 8, 3), dev)
  with pytest.raises(ValueError, match='out must be a float32'):
    ingest.resize_area_f32(d, (4, 3), out=torch.empty((3, 4, 3), dtype=torch.uint8, device=dev))
  with pytest.raises(ValueError, match='must be float32'):  # the float form takes float32 only ...
    ingest.resize_area_f32(ic.dev_t(ic.u8_image(6, 8, 3), dev), (4, 3))
  with pytest.raises(ValueError, match='must be uint8'):    # ... and resize_area stays the uint8 form
    ingest.resize_area(d, (4, 3))
  u8 = ic.dev_t(ic.u8_image(6, 8, 3), dev)
  for size in ((9, 6), (8, 7)):  # uint8 enlarging: refused as before, with the old message
    with pytest.raises(ValueError, match=r'resize_area shrinks: 6 x 8 -> .* enlarges an axis \(the reference only shrinks with INTER_AREA\)'):
      ingest.resize_area(u8, size)
  assert tuple(ingest.resize_area_f32(d, (9, 7)).shape) == (7, 9, 3)  # float32 enlarges
  # the C entry refuses what Python refuses, by itself
  from dynibar_amd import _lib
  out = torch.empty((3, 4, 5), dtype=torch.float32, device=dev)
  five = ic.dev_t(f01_image(6, 8, 5), dev)
  with pytest.raises(RuntimeError, match='C=5 is unsupported'):
    _lib.call('dyn_resize_area_f32', 1, 6, 8, 5, 3, 4, five.data_ptr(), out.data_ptr(), 3 * 4 * 5 * 4, None, None, None, 0, None, None, None, 0,
              _lib.stream_of(five))


# ---- the batched virtual views -------------------------------------------------------------------------------------------------------
def vv_frame(f, H, W, near=False):
  """a smooth image and a disparity with a step (a near disc on a far background), as _frame of tests/test_gpu_virtual_views.py builds them, at
  H x W; ``near``: a few pixels so close that some views are translated past them (Q.z <= 0)"""
  yy, xx = np.mgrid[0:H, 0:W]
  s = W / 512.0
  img = np.clip(0.5 + 0.4 * np.sin(xx / (17.0 * s) + f)[..., None] * np.cos(yy[..., None] / (11.0 * s) + np.arange(3)), 0, 1).astype(F32)
  cx, cy, r = W * (0.4 + 0.1 * f), H * 0.5, H * 0.22
  # (the step is large enough that the Sobel alpha falls below 0.5 along the disc's rim: depth 8 -> 2 is |grad| ~ 2.4 of depth / 10)
  disp = (0.12 + 0.02 * np.sin(xx / (53.0 * s)) * np.cos(yy / (31.0 * s)) + 0.4 * (((xx - cx) ** 2 + (yy - cy) ** 2) < r ** 2)).astype(F32)
  if near:
    disp[H // 3, W // 3:W // 3 + 3] = 40.0
  return img, disp


@functools.lru_cache(maxsize=None)
def vv_inputs(F=3, H=24, W=40, near=False, shift=4.0):
  """-> (img [F,H,W,3], disp [F,H,W], K [3,3], c2w [F,4,4], vv_c2w [F,8,3,4]); the bounds handed to virtual_view_poses make the largest pixel
  shift about ``shift`` px: it is 63 * bound / depth whatever the image size (84 * 0.75 * bound / focal of camera motion, times focal / depth)"""
  from dynibar_amd import virtual_views as vv
  frames = [vv_frame(f, H, W) for f in range(F)]
  if near:
    frames[-1] = vv_frame(F - 1, H, W, near=True)
  img, disp = np.stack([x[0] for x in frames]), np.stack([x[1] for x in frames])
  focal = 0.9 * W
  K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], F32)
  rng = np.random.RandomState(6)
  c2w = np.tile(np.eye(4), (F, 1, 1))
  c2w[:, :3, 3] = rng.uniform(-0.2, 0.2, (F, 3))
  nearest = min(float(1.0 / vv_frame(f, H, W)[1].max()) for f in range(F))  # (of the scene without the near pixels)
  bounds = [shift / 63.0 * nearest] * F
  hwf = np.array([H, W, focal]).reshape([3, 1])
  _, vsv = vv.virtual_view_poses([c.astype(F32) for c in c2w], bounds, hwf)
  return img, disp, K, c2w, vsv


def yardstick(img, disp, K, c2w, vsv):
  """the per-frame path -> uint8 [F, V, H, W, 3] on the host"""
  from dynibar_amd import virtual_views as vv
  return np.stack([vv.render_frame_virtual_views(img[f], disp[f], K, c2w[f], vsv[f]) for f in range(len(img))])


@functools.lru_cache(maxsize=None)
def shared_yardstick(dev):
  """the yardstick of vv_inputs(), rendered once per device for the checks that compare with it; they leave it unchanged"""
  img, disp, K, c2w, vsv = vv_inputs()
  return yardstick(ic.dev_t(img, dev), ic.dev_t(disp, dev), K, c2w, vsv)


def interior_holes(view):
  """black pixels with rendered pixels on both sides in their row AND in their column: holes inside the rendered region (disocclusions and
  what the erosion took around them), not the band a view's shift empties along the image border"""
  on = view.max(-1) > 0
  left = np.maximum.accumulate(on, axis=1)
  right = np.maximum.accumulate(on[:, ::-1], axis=1)[:, ::-1]
  up = np.maximum.accumulate(on, axis=0)
  down = np.maximum.accumulate(on[::-1], axis=0)[::-1]
  return int(np.sum(~on & left & right & up & down))


def assert_not_vacuous(views):
  """on the YARDSTICK's output: every view is between 30 % and 98 % rendered, and some view has an interior hole"""
  F, V = views.shape[:2]
  fill = (views.max(-1) > 0).reshape(F * V, -1).mean(1)
  assert fill.min() > 0.30 and fill.max() < 0.98, fill
  assert max(interior_holes(v) for v in views.reshape((F * V,) + views.shape[2:])) > 0


def behind_camera(disp, K, c2w, vsv):
  """how many (pixel, view) pairs of the last frame have Q.z <= 0, in float64"""
  from dynibar_amd import ingest
  rot, tr = ingest.relative_transforms(c2w[-1:], vsv[-1:])
  H, W = disp.shape[1:]
  yy, xx = np.mgrid[0:H, 0:W]
  P = (1.0 / disp[-1].astype(np.float64))[None] * (np.linalg.inv(K.astype(np.float64)) @ np.stack([xx, yy, np.ones_like(xx)]).reshape(3, -1).astype(np.float64)).reshape(3, H, W)
  z = np.einsum('vj,jhw->vhw', rot[0, :, 2, :], P) + tr[0, :, 2, None, None]
  return int(np.sum(z <= 0))


def check_views_equal_the_per_frame_path(dev):
  from dynibar_amd import ingest
  img, disp, K, c2w, vsv = vv_inputs()
  want = shared_yardstick(dev)
  assert want.shape == VV_SHAPE + (3,) and want.dtype == np.uint8
  assert_not_vacuous(want)
  di, dd = ic.dev_t(img, dev), ic.dev_t(disp, dev)
  ingest.virtual_views(di, dd, K, c2w, vsv)  # (the first call allocates the workspace)
  with ic.no_sync(dev):
    got = ingest.virtual_views(di, dd, K, c2w, vsv)
  assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
  g = ic.host(got)
  assert np.array_equal(g, want), f'{int(np.sum(g != want))} bytes differ'
  for batch in (1, 2, 3):
    assert np.array_equal(ic.host(ingest.virtual_views(di, dd, K, c2w, vsv, batch=batch)), want), batch
  # a second call with another F on the same workspace: the shared frames keep their bytes
  assert np.array_equal(ic.host(ingest.virtual_views(di[:2], dd[:2], K, c2w[:2], vsv[:2])), want[:2])
  assert np.array_equal(ic.host(ingest.virtual_views(di, dd, K, c2w, vsv)), want)
  # per-frame intrinsics [N, 3, 3], and a store with spaced views
  assert np.array_equal(ic.host(ingest.virtual_views(di, dd, np.stack([K] * 3), c2w, vsv)), want)
  n = 24 * 40 * 3
  store = torch.full((3 * 8, n + 16), 0xA5, dtype=torch.uint8, device=dev)
  view = store[:, :n].view(3, 8, 24, 40, 3)
  assert ingest.virtual_views(di, dd, K, c2w, vsv, out=view, batch=2) is view
  s = ic.host(store)
  assert np.array_equal(s[:, :n].reshape(want.shape), want) and (s[:, n:] == 0xA5).all()


def check_per_frame_intrinsics_that_differ(dev):
  """every frame with its own focal length and principal point: the batched projection must read K and K^-1 of frame b / V, not of entry b
  or of frame 0 (three copies of one K, as above, cannot tell)"""
  from dynibar_amd import ingest, virtual_views as vv
  img, disp, K, c2w, vsv = vv_inputs()
  Ks = np.stack([K] * 3)
  for f, (scale, dx, dy) in enumerate(((0.9, -1.5, 1.0), (1.0, 0.0, 0.0), (1.1, 2.0, -1.25))):
    Ks[f, 0, 0] *= F32(scale)
    Ks[f, 1, 1] *= F32(scale)
    Ks[f, 0, 2] += F32(dx)
    Ks[f, 1, 2] += F32(dy)
  di, dd = ic.dev_t(img, dev), ic.dev_t(disp, dev)
  want = np.stack([vv.render_frame_virtual_views(di[f], dd[f], Ks[f], c2w[f], vsv[f]) for f in range(3)])
  assert_not_vacuous(want)
  assert all(int(np.sum(want[f] != shared_yardstick(dev)[f])) > 1000 for f in (0, 2))  # (the intrinsics matter to the bytes)
  g = ic.host(ingest.virtual_views(di, dd, Ks, c2w, vsv))
  assert np.array_equal(g, want), [int(np.sum(g[f] != want[f])) for f in range(3)]


def check_more_than_one_sort_group(dev):
  """At 8 views of 24 x 40 a sort group of dyn_vv_frames holds 8 frames, so a call of nine runs the group loop twice, the second time for
  frame 8 alone at the offsets of f0 = 8.  The nine frames are the three of vv_inputs() in turn: frame 8 is frame 2, whose bytes are neither
  frame 0's nor frame 1's."""
  from dynibar_amd import _lib, ingest
  img, disp, K, c2w, vsv = vv_inputs()
  want = shared_yardstick(dev)
  sizes = [int(_lib.lib().dyn_vv_frames_workspace_bytes(F, 8, 24, 40)) for F in (7, 8, 9)]
  assert sizes[0] < sizes[1] == sizes[2], sizes  # a group is 8 frames
  assert min(int(np.sum(want[2] != want[f])) for f in (0, 1)) > 21000
  idx = np.arange(9) % 3
  got = ingest.virtual_views(ic.dev_t(img[idx], dev), ic.dev_t(disp[idx], dev), K, c2w[idx], vsv[idx], batch=9)
  g = ic.host(got)
  assert np.array_equal(g, want[idx]), [int(np.sum(g[i] != want[idx[i]])) for i in range(9)]


def check_one_frame_one_view(dev):
  from dynibar_amd import ingest
  img, disp, K, c2w, vsv = vv_inputs()
  want = yardstick(ic.dev_t(img[1:2], dev), ic.dev_t(disp[1:2], dev), K, c2w[1:2], vsv[1:2, 5:6])
  got = ingest.virtual_views(ic.dev_t(img[1:2], dev), ic.dev_t(disp[1:2], dev), K, c2w[1:2], vsv[1:2, 5:6])
  assert tuple(got.shape) == (1, 1, 24, 40, 3) and np.array_equal(ic.host(got), want)
  assert 0.30 < (want.max(-1) > 0).mean() < 0.98


def check_points_behind_the_camera(dev):
  from dynibar_amd import ingest
  img, disp, K, c2w, vsv = vv_inputs(near=True)
  assert behind_camera(disp, K, c2w, vsv) > 0
  want = yardstick(ic.dev_t(img, dev), ic.dev_t(disp, dev), K, c2w, vsv)
  got = ingest.virtual_views(ic.dev_t(img, dev), ic.dev_t(disp, dev), K, c2w, vsv)
  assert np.array_equal(ic.host(got), want), f'{int(np.sum(ic.host(got) != want))} bytes differ'
  assert (want[-1].max(-1) > 0).mean() > 0.30


def check_views_refusals(dev):
  import pytest
  from dynibar_amd import ingest
  img, disp, K, c2w, vsv = vv_inputs()
  di, dd = ic.dev_t(img, dev), ic.dev_t(disp, dev)
  with pytest.raises(ValueError, match='disp must be'):
    ingest.virtual_views(di, dd[:2], K, c2w, vsv)
  with pytest.raises(ValueError, match='vv_c2w'):
    ingest.virtual_views(di, dd, K, c2w, vsv[:2])
  with pytest.raises(ValueError, match='batch'):
    ingest.virtual_views(di, dd, K, c2w, vsv, batch=0)
  with pytest.raises(ValueError, match='out must be'):
    ingest.virtual_views(di, dd, K, c2w, vsv, out=torch.empty((3, 8, 24, 40, 3), dtype=torch.float32, device=dev))
