"""Support for the scene-preparation tests (dynibar_amd/ingest.py, csrc/dyn_ingest.h): seeded inputs, numpy restatements of the contracts in
include/dynibar_hip.h (scene preparation), the independent definitions the restatements are pinned to (tests/test_ingest_cpu.py) and the checks
the device and the emulator tests share.  Test infrastructure: nothing in dynibar_amd imports this.

The restatements are written from the contract, not from dynibar_amd/ingest.py: they build their own tables.  numpy's float32 operations
are single IEEE operations, which is what "one rounded operation at a time" asks for.  Every device comparison is exact."""
import contextlib
import functools
import math

import numpy as np
import torch

F32 = np.float32
# (Hs, Ws, Hd, Wd): table branch with both axes partial; the 2 x 2 branch; 3 x 2 with the float scale; one axis a copy and the other slivers near
# the 1e-3 rule; the copy
AREA_SHAPES = [(15, 23, 4, 6), (8, 12, 4, 6), (12, 12, 4, 6), (3, 1001, 3, 1000), (7, 9, 7, 9)]
AREA_CPU_SHAPES = AREA_SHAPES[:4] + [(30, 46, 8, 13), (108, 192, 29, 51)]
AREA_TIE_SEED = 3
AREA_TIE_CASE = (30, 46, 8, 13, 3)  # with that seed: a table-branch case whose sums hit k + 0.5 with k even (half-up and half-even part ways)
LINEAR_SHAPES = [(2, 3, 5, 7), (9, 13, 4, 5), (6, 7, 6, 7)]
PRODUCTION = (1080, 1920, 288, 512)
DEPTH_SHAPE = (384, 672)
ERODE_SHAPES = [(3, 3), (7, 9), (33, 40), (288, 512)]  # smaller than the footprint; one tile; a width off the tile of 64; the erosion's size
ERODE_EMU_SHAPES = ERODE_SHAPES[:3] + [(35, 67)]       # ... and more than one tile each way at a size the emulator can afford
ERODE_RADII = [0, 1, 3, 5, 15]
DENSITIES = [0.5, 0.9, 0.98]
PLAN_SIZES = (1, 2, 19, 20, 21, 100, 258048)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def u8_image(*shape, seed=0):
  return np.random.default_rng([seed, 11] + list(shape)).integers(0, 256, shape, dtype=np.uint8)


def f32_image(*shape, seed=0):
  return (np.random.default_rng([seed, 12] + list(shape)).random(shape) * 4.5 + 0.5).astype(F32)


def mask01(*shape, density=0.9, seed=0):
  return (np.random.default_rng([seed, 13] + list(shape)).random(shape) < density).astype(np.uint8)


def raw_mask(*shape, seed=0):
  """a decoded mask file: mostly 0 and 255, some 1 and 254 (both sides of the loader's threshold)"""
  rng = np.random.default_rng([seed, 14] + list(shape))
  blobs = rng.random(shape) < 0.8
  return np.where(blobs, 255, rng.choice(np.array([0, 0, 0, 1, 254], dtype=np.uint8), shape)).astype(np.uint8)


# ---- the restatements ----------------------------------------------------------------------------------------------------------------
def axis_scale(s, d):
  return 1.0 / (float(d) / s)


def decimation_table(s, d):
  """-> per destination index the list of (source index, float32 weight)"""
  scale = axis_scale(s, d)
  tab = []
  for i in range(d):
    f1 = i * scale
    f2 = f1 + scale
    cell = min(scale, s - f1)
    s1 = int(math.ceil(f1))
    s2 = min(int(math.floor(f2)), s - 1)
    s1 = min(s1, s2)
    row = []
    if s1 - f1 > 1e-3:
      row.append((s1 - 1, F32((s1 - f1) / cell)))
    for k in range(s1, s2):
      row.append((k, F32(1.0 / cell)))
    if f2 - s2 > 1e-3:
      row.append((s2, F32(min(min(f2 - s2, 1.0), cell) / cell)))
    tab.append(row)
  return tab


def area_is_integer(Hs, Ws, Hd, Wd):
  eps = np.finfo(np.float64).eps
  sx, sy = axis_scale(Ws, Wd), axis_scale(Hs, Hd)
  return abs(sx - int(sx)) < eps and abs(sy - int(sy)) < eps


def area_sums(src, size):
  """the value before rounding: the integer sum of the block (int64) in the integer branch, the fp32 sum in the table branch -> (values, branch)"""
  src = src[:, :, None] if src.ndim == 2 else src
  Hs, Ws, C = src.shape
  Wd, Hd = size
  if area_is_integer(Hs, Ws, Hd, Wd):
    ix, iy = int(axis_scale(Ws, Wd)), int(axis_scale(Hs, Hd))
    return src.astype(np.int64).reshape(Hd, iy, Wd, ix, C).sum(axis=(1, 3)), (ix, iy)
  xt, yt = decimation_table(Ws, Wd), decimation_table(Hs, Hd)
  S = src.astype(F32)
  rows = np.zeros((Hs, Wd, C), F32)
  for dx, row in enumerate(xt):
    acc = np.zeros((Hs, C), F32)
    for k, a in row:
      acc = acc + S[:, k, :] * a
    rows[:, dx, :] = acc
  out = np.zeros((Hd, Wd, C), F32)
  for dy, row in enumerate(yt):
    acc = None
    for k, b in row:
      t = b * rows[k]
      acc = t if acc is None else acc + t
    out[dy] = acc
  return out, None


def resize_area(src, size):
  """dyn_resize_area_u8 for one image: uint8 [H, W] or [H, W, C], size = (width, height)"""
  v, block = area_sums(src, size)
  if block is not None:
    ix, iy = block
    if ix == 2 and iy == 2:
      out = (v + 2) >> 2
    else:
      out = np.rint(v.astype(F32) * (F32(1) / F32(ix * iy)))
  else:
    out = np.rint(v)  # ties to even
  out = np.clip(out, 0, 255).astype(np.uint8)
  return out[:, :, 0] if src.ndim == 2 else out


def table_ties(src, size):
  """how many values of the table branch sit exactly on k + 0.5 with k even: where round-half-up and ties-to-even give different bytes"""
  v, block = area_sums(src, size)
  assert block is None
  k = np.floor(v)
  return int(np.sum((v - k == F32(0.5)) & (k % 2 == 0) & (v < 255)))


def _linear_axis(s, d):
  i = np.arange(d, dtype=np.float64)
  f = ((i + 0.5) * axis_scale(s, d) - 0.5).astype(F32)
  s0 = np.floor(f)
  f = f - s0
  return s0.astype(np.int64), f.astype(F32)


def resize_linear(src, size, dtype=F32):
  """dyn_resize_linear_f32 for one image (dtype=np.float64: the same formula with the same fp32 coordinates, evaluated in double)"""
  Hs, Ws = src.shape
  Wd, Hd = size
  S = src.astype(dtype)
  one = dtype(1)
  sx, fx = _linear_axis(Ws, Wd)
  fx = np.where(sx < 0, F32(0), fx)
  sx = np.where(sx < 0, 0, sx)
  edge = sx >= Ws - 1
  a = np.minimum(sx, Ws - 1)
  b = np.minimum(a + 1, Ws - 1)
  fxd = fx.astype(dtype)
  rows = np.where(edge[None, :], S[:, a], S[:, a] * (one - fxd)[None, :] + S[:, b] * fxd[None, :]).astype(dtype)
  sy, fy = _linear_axis(Hs, Hd)
  r0, r1 = np.clip(sy, 0, Hs - 1), np.clip(sy + 1, 0, Hs - 1)
  fyd = fy.astype(dtype)
  return (rows[r0] * (one - fyd)[:, None] + rows[r1] * fyd[:, None]).astype(dtype)


def nearest_index(s, d):
  return np.minimum(np.floor(np.arange(d, dtype=np.float64) * axis_scale(s, d)).astype(np.int64), s - 1)


def resize_nearest(src, size, below=None):
  Wd, Hd = size
  out = src[nearest_index(src.shape[0], Hd)][:, nearest_index(src.shape[1], Wd)]
  if below is not None:
    first = out.reshape(Hd, Wd, -1).view(np.uint8)[:, :, 0]
    return (first < below).astype(np.uint8)
  return np.ascontiguousarray(out)


def erode_disk(mask, r):
  """the AND over the in-image taps of the disk, tap by tap"""
  H, W = mask.shape
  m = mask != 0
  out = np.ones((H, W), bool)
  for dy in range(-r, r + 1):
    for dx in range(-r, r + 1):
      if dx * dx + dy * dy > r * r or abs(dy) >= H or abs(dx) >= W:  # (outside the disk, or no tap of this offset lies in the image)
        continue
      ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))   # the (y, x) whose tap (y + dy, x + dx) is in the image
      yt, xt = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
      out[ys, xs] &= m[yt, xt]
  return out.astype(np.uint8)


def erosion_size(size):
  return int(round(288.0 * size[0] / size[1])), 288


def motion_mask(raw, size, radius):
  """monocular.py:168-203 on the decoded file, with the restatements"""
  small = resize_nearest(raw, erosion_size(size), below=255)
  return resize_nearest(erode_disk(small, radius), size)


def static_mask(raw, size):
  return resize_nearest(raw, size, below=255)


def disparity(depth, size, scale):
  return resize_linear(F32(1) / depth, size) / F32(scale)


def depth_bounds(depth, q=(5, 95)):
  """numpy itself, one scalar call per percentile as the script has them"""
  return np.array([np.percentile(depth, q[0]), np.percentile(depth, q[1])])


# ---- independent definitions ---------------------------------------------------------------------------------------------------------
def box_average(src, size):
  """the float64 average of the source over each destination cell (partial pixels by their covered fraction)"""
  src = src[:, :, None] if src.ndim == 2 else src
  Wd, Hd = size

  def weights(s, d):
    scale = s / d
    w = np.zeros((d, s))
    for i in range(d):
      lo, hi = i * scale, (i + 1) * scale
      for k in range(int(math.floor(lo)), min(s, int(math.ceil(hi)))):
        w[i, k] = max(0.0, min(hi, k + 1) - max(lo, k)) / scale
    return w

  wy, wx = weights(src.shape[0], Hd), weights(src.shape[1], Wd)
  return np.einsum('ik,klc,jl->ijc', wy, src.astype(np.float64), wx)


def area_bound(Hs, Ws, Hd, Wd):
  """rounding + the slivers the 1e-3 rule skips + the fp32 sums"""
  return 0.5 + 255 * (2e-3 / (Ws / Wd) + 2e-3 / (Hs / Hd)) + 1e-3


def plan_percentile(x, rank, weight):
  """numpy's _lerp on the plan's order statistics, in the weight's dtype against float32 data"""
  s = np.sort(x.reshape(-1))
  out = []
  for (lo, hi), t in zip(rank, weight):
    a, b = s[lo], s[hi]
    d = b - a
    out.append(b - d * (1 - t) if t >= 0.5 else a + d * t)
  return out


# ---- shared device checks ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def no_sync(dev):
  """a host synchronisation inside raises (HIP devices only: the emulator has no streams)"""
  if torch.device(dev).type != 'cuda':
    yield
    return
  torch.cuda.set_sync_debug_mode('error')
  try:
    yield
  finally:
    torch.cuda.set_sync_debug_mode('default')


def dev_t(x, dev):
  return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def host(t):
  return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def production_area():
  src = u8_image(PRODUCTION[0], PRODUCTION[1], 3, seed=5)
  return src, resize_area(src, (PRODUCTION[3], PRODUCTION[2]))


def check_area(dev, Hs, Ws, Hd, Wd, C, seed=0):
  from dynibar_amd import ingest
  src = u8_image(Hs, Ws, C, seed=seed)
  want = resize_area(src, (Wd, Hd))
  d = dev_t(src, dev)
  ingest.resize_area(d, (Wd, Hd))  # (the first call of a size uploads its tables)
  with no_sync(dev):
    got = ingest.resize_area(d, (Wd, Hd))
    again = ingest.resize_area(d, (Wd, Hd))
  assert got.dtype == torch.uint8 and tuple(got.shape) == (Hd, Wd, C)
  assert np.array_equal(host(got), want), f'{int(np.sum(host(got) != want))} bytes differ'
  assert torch.equal(got, again)
  if C == 1:  # the [H, W] form and a host array
    assert np.array_equal(host(ingest.resize_area(src[:, :, 0], (Wd, Hd), device=dev)), want[:, :, 0])


def check_area_pitched(dev, Hs=15, Ws=23, Hd=4, Wd=6, C=3, B=3, pad=13):
  """B images into a store whose rows are longer than an image: the padding keeps its bytes, also where a row starts off 4 bytes"""
  from dynibar_amd import ingest
  src = u8_image(B, Hs, Ws, C, seed=3)
  nbytes = Hd * Wd * C
  store = torch.full((B, nbytes + pad), 0xA5, dtype=torch.uint8, device=dev)
  view = store[:, :nbytes].view(B, Hd, Wd, C)
  ret = ingest.resize_area(dev_t(src, dev), (Wd, Hd), out=view)
  assert ret is view
  got = host(store)
  for b in range(B):
    assert np.array_equal(got[b, :nbytes].reshape(Hd, Wd, C), resize_area(src[b], (Wd, Hd))), b
  assert (got[:, nbytes:] == 0xA5).all(), 'the padding was written'


def check_area_production(dev):
  from dynibar_amd import ingest
  src, want = production_area()
  got = ingest.resize_area(dev_t(src, dev), (PRODUCTION[3], PRODUCTION[2]))
  assert np.array_equal(host(got), want), f'{int(np.sum(host(got) != want))} bytes differ'


def check_area_refusals(dev):
  import pytest
  from dynibar_amd import ingest
  d = dev_t(u8_image(6, 8, 3), dev)
  with pytest.raises(ValueError, match='enlarges'):
    ingest.resize_area(d, (9, 6))
  with pytest.raises(ValueError, match='enlarges'):
    ingest.resize_area(d, (8, 7))
  with pytest.raises(ValueError):
    ingest.resize_area(d.float(), (4, 3))
  with pytest.raises(ValueError):
    ingest.resize_area(dev_t(u8_image(6, 8, 2), dev), (4, 3))
  with pytest.raises(ValueError):
    ingest.resize_area(d, (0, 3))
  with pytest.raises(ValueError):
    ingest.erode_disk(dev_t(mask01(5, 5), dev), 16)
  with pytest.raises(ValueError):
    ingest.resize_nearest(dev_t(np.zeros((4, 4, 4), F32), dev), (2, 2))
  with pytest.raises(ValueError):
    ingest.resize_linear(d, (4, 3))
  # the C entry refuses an enlarging call by itself, with a message
  from dynibar_amd import _lib
  out = torch.empty((7, 8, 3), dtype=torch.uint8, device=dev)
  with pytest.raises(RuntimeError, match='enlarges an axis'):
    _lib.call('dyn_resize_area_u8', 1, 6, 8, 3, 7, 8, d.data_ptr(), out.data_ptr(), 7 * 8 * 3, None, None, None, 0, None, None, None, 0,
              _lib.stream_of(d))


def check_linear(dev, Hs, Ws, Hd, Wd, B=None, seed=0):
  from dynibar_amd import ingest
  src = f32_image(*((Hs, Ws) if B is None else (B, Hs, Ws)), seed=seed)
  d = dev_t(src, dev)
  with no_sync(dev):
    got = ingest.resize_linear(d, (Wd, Hd))
    again = ingest.resize_linear(d, (Wd, Hd))
  want = resize_linear(src, (Wd, Hd)) if B is None else np.stack([resize_linear(s, (Wd, Hd)) for s in src])
  assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
  assert np.array_equal(host(got).view(np.uint32), want.view(np.uint32)), f'{int(np.sum(host(got) != want))} values differ'
  assert torch.equal(got, again)
  if (Hs, Ws) == (Hd, Wd):
    assert np.array_equal(host(got).view(np.uint32), src.view(np.uint32))


def check_nearest(dev, src, size, below=None):
  from dynibar_amd import ingest
  d = dev_t(src, dev)
  with no_sync(dev):
    got = ingest.resize_nearest(d, size, below=below)
    again = ingest.resize_nearest(d, size, below=below)
  want = resize_nearest(src, size, below=below)
  assert str(got.dtype).replace('torch.', '') == str(want.dtype) and tuple(got.shape) == want.shape, (got.dtype, got.shape, want.shape)
  assert np.array_equal(host(got).view(np.uint8), want.view(np.uint8))
  assert torch.equal(got, again)


def check_nearest_cases(dev):
  check_nearest(dev, u8_image(5, 7), (5, 7))            # 5 x 7 -> 7 x 5 (size is width, height)
  check_nearest(dev, u8_image(5, 7, 3), (5, 7))
  check_nearest(dev, f32_image(5, 7, 2), (5, 7))
  for src in (u8_image(5, 7), u8_image(5, 7, 3), f32_image(5, 7, 2)):  # the identity
    check_nearest(dev, src, (7, 5))
  vals = np.array([0, 1, 254, 255], dtype=np.uint8)
  check_nearest(dev, vals[np.random.default_rng(3).integers(0, 4, (9, 11))], (6, 5), below=255)
  check_nearest(dev, vals[np.random.default_rng(4).integers(0, 4, (9, 11, 3))], (13, 9), below=255)


def check_erode(dev, H, W, r, density, seed=0):
  from dynibar_amd import ingest
  m = mask01(H, W, density=density, seed=seed)
  d = dev_t(m, dev)
  with no_sync(dev):
    got = ingest.erode_disk(d, r)
    again = ingest.erode_disk(d, r)
  assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W)
  assert np.array_equal(host(got), erode_disk(m, r)), f'{H} x {W}, r = {r}'
  assert torch.equal(got, again)
  if r == 0:
    assert np.array_equal(host(got), m)


def check_erode_special(dev, H=33, W=40):
  from dynibar_amd import ingest
  ones = np.ones((2, H, W), np.uint8)
  for r in (1, 5, 15):  # all ones stays all ones: the border does not erode
    assert np.array_equal(host(ingest.erode_disk(dev_t(ones, dev), r)), ones), r
  for r, (cy, cx) in ((3, (16, 20)), (5, (2, 37)), (15, (30, 1))):  # a single zero erases exactly the disk around it
    m = np.ones((H, W), np.uint8)
    m[cy, cx] = 0
    yy, xx = np.mgrid[0:H, 0:W]
    want = ((yy - cy) ** 2 + (xx - cx) ** 2 > r * r).astype(np.uint8)
    assert np.array_equal(host(ingest.erode_disk(dev_t(m, dev), r)), want), (r, cy, cx)
  # a batch into a pitched store
  m = mask01(3, H, W, density=0.95, seed=9)
  store = torch.full((3, H * W + 7), 0xA5, dtype=torch.uint8, device=dev)
  ingest.erode_disk(dev_t(m, dev), 3, out=store[:, :H * W].view(3, H, W))
  got = host(store)
  for b in range(3):
    assert np.array_equal(got[b, :H * W].reshape(H, W), erode_disk(m[b], 3))
  assert (got[:, H * W:] == 0xA5).all()
  assert np.array_equal(host(ingest.erode_disk(dev_t(m[0].astype(bool), dev), 3)), erode_disk(m[0], 3))  # bool input


def bounds_data(name, n):
  rng = np.random.default_rng([n, 15])
  if name == 'uniform':
    x = rng.random(n) * 9.0 + 0.3
  elif name == 'all_equal':
    x = np.full(n, 2.75)
  elif name == 'signed_zeros':
    x = np.where(rng.random(n) < 0.3, rng.choice(np.array([-0.0, 0.0]), n), rng.standard_normal(n))
  elif name == 'mostly_zeros':  # nine values in ten a zero of either sign: the 5th percentile IS a zero
    x = np.where(rng.random(n) < 0.9, rng.choice(np.array([-0.0, 0.0]), n), rng.random(n) + 0.5)
  else:
    raise KeyError(name)
  return np.asarray(x, dtype=F32)


def check_bounds(dev, shape, name, batch=None):
  from dynibar_amd import ingest
  n = int(np.prod(shape))
  x = bounds_data(name, n * (batch or 1)).reshape(((batch,) if batch else ()) + tuple(shape))
  d = dev_t(x, dev)
  with no_sync(dev):
    got = ingest.depth_bounds(d)
    again = ingest.depth_bounds(d)
  want = depth_bounds(x) if batch is None else np.stack([depth_bounds(v) for v in x])
  g = host(got)
  assert g.dtype == want.dtype == F32 and g.shape == want.shape, (g.dtype, want.dtype, g.shape)
  assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (g, want)
  assert torch.equal(got, again)


def check_bounds_on_a_zero(dev, shape=(33, 31)):
  """A selected order statistic that is a zero: the VALUES equal numpy's, the sign of the zero is unspecified (ingest.depth_bounds: the
  selection folds -0.0 into +0.0 and returns +0.0; numpy returns whichever zero its partition left at the rank).  The other percentile is
  compared in bits as everywhere."""
  from dynibar_amd import ingest
  x = bounds_data('mostly_zeros', int(np.prod(shape))).reshape(shape)
  want = depth_bounds(x)
  assert want[0] == 0 and want[1] > 0.5, want
  got = host(ingest.depth_bounds(dev_t(x, dev)))
  assert got.dtype == F32 and got[0] == 0 and not np.signbit(got[0]), got   # +0.0, whatever sign numpy's zero has
  assert got[1:].view(np.uint32) == want[1:].view(np.uint32)
  allneg = np.full(shape, -0.0, F32)
  got = host(ingest.depth_bounds(dev_t(allneg, dev)))
  assert (got == 0).all() and (depth_bounds(allneg) == 0).all()


def check_chain_refusals(dev):
  import pytest
  from dynibar_amd import ingest
  rgb = dev_t(raw_mask(9, 11, 3), dev)
  for call in (lambda: ingest.motion_mask(rgb, (6, 5), 1), lambda: ingest.static_mask(rgb, (6, 5)),
               lambda: ingest.static_mask(dev_t(raw_mask(9, 11, 4), dev), (6, 5))):
    with pytest.raises(ValueError, match='colour channels'):
      call()
  assert np.array_equal(host(ingest.static_mask(rgb[..., 0], (6, 5))), static_mask(host(rgb)[..., 0], (6, 5)))  # channel 0, as the loader reads it
  # sizes the kernels' grids cannot hold are refused by the Python checks, as ValueError
  with pytest.raises(ValueError, match='too large'):
    ingest.erode_disk(torch.zeros((65536, 1), dtype=torch.uint8, device=dev), 1)
  with pytest.raises(ValueError, match='too large'):
    ingest.resize_area(torch.zeros((65536, 1, 1), dtype=torch.uint8, device=dev), (1, 65536))
  # out= of the chains
  raw = raw_mask(2, 37, 53, seed=1)
  mm = torch.full((2, 16, 23), 7, dtype=torch.uint8, device=dev)
  sm = torch.full((2, 16, 23), 7, dtype=torch.uint8, device=dev)
  assert ingest.motion_mask(dev_t(raw, dev), (23, 16), 2, out=mm) is mm and ingest.static_mask(dev_t(raw, dev), (23, 16), out=sm) is sm
  for b in range(2):
    assert np.array_equal(host(mm)[b], motion_mask(raw[b], (23, 16), 2)) and np.array_equal(host(sm)[b], static_mask(raw[b], (23, 16)))
  one = torch.full((16, 23), 7, dtype=torch.uint8, device=dev)
  ingest.static_mask(dev_t(raw[0], dev), (23, 16), out=one)
  assert np.array_equal(host(one), static_mask(raw[0], (23, 16)))


def check_chains(dev, Hs=37, Ws=53, size=(23, 16), radius=3, B=2):
  from dynibar_amd import ingest
  raw = raw_mask(B, Hs, Ws, seed=1)
  d = dev_t(raw, dev)
  with no_sync(dev):
    mm = ingest.motion_mask(d, size, radius)
    sm = ingest.static_mask(d, size)
  for b in range(B):
    assert np.array_equal(host(mm)[b], motion_mask(raw[b], size, radius)), b
    assert np.array_equal(host(sm)[b], static_mask(raw[b], size)), b
  assert np.array_equal(host(ingest.motion_mask(d[0], size, radius)), motion_mask(raw[0], size, radius))  # one frame
  depth = f32_image(B, 29, 41, seed=2)
  dd = dev_t(depth, dev)
  with no_sync(dev):
    disp = ingest.disparity(dd, size, 1.7)
  for b in range(B):
    assert np.array_equal(host(disp)[b].view(np.uint32), disparity(depth[b], size, 1.7).view(np.uint32)), b
  assert disp.dtype == torch.float32


# ---- a whole scene -------------------------------------------------------------------------------------------------------------------
def decoded_scene(N=7, Hs=37, Ws=53, size=(23, 16), seed=0):
  """what a caller has after decoding the files of a scene -> (the arguments of prepare_monocular / from_decoded, size)"""
  W, H = size
  rng = np.random.default_rng([seed, 16])
  poses = np.tile(np.eye(4), (N, 1, 1))
  poses[:, :3, 3] = rng.standard_normal((N, 3)) * 0.1
  intr = np.tile(np.array([[20.0, 0, W / 2, 0], [0, 20.0, H / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]]), (N, 1, 1))
  vposes = np.tile(np.eye(4), (N, 8, 1, 1))
  vposes[:, :, :3, 3] = rng.standard_normal((N, 8, 3)) * 0.1
  return dict(frames=u8_image(N, Hs, Ws, 3, seed=seed), depth=f32_image(N, 29, 41, seed=seed), dynamic_masks=raw_mask(N, Hs, Ws, seed=seed),
              static_masks=raw_mask(N, Hs, Ws, seed=seed + 1), flows=(rng.standard_normal((N, 6, H, W, 2)) * 3).astype(F32),
              flow_masks=(rng.random((N, 6, H, W)) < 0.8).astype(F32), virtual_views=u8_image(N, 8, H, W, 3, seed=seed + 2), virtual_poses=vposes,
              intrinsics=intr, poses=poses, depth_range=(0.5, 9.0), scale=1.3, erosion_radius=2, size=size)


def host_prepared(dec):
  """the constructor's arguments from the restatements, on the host"""
  size, N = dec['size'], len(dec['frames'])
  return dict(images=np.stack([resize_area(f, size) for f in dec['frames']]), intrinsics=dec['intrinsics'], poses=dec['poses'],
              depth_range=dec['depth_range'], disp=np.stack([disparity(d, size, dec['scale']) for d in dec['depth']]),
              motion_mask=np.stack([motion_mask(m, size, dec['erosion_radius']) for m in dec['dynamic_masks']]),
              static_mask=np.stack([static_mask(m, size) for m in dec['static_masks']]), flows=dec['flows'], flow_masks=dec['flow_masks'],
              virtual_views=dec['virtual_views'], virtual_poses=dec['virtual_poses'])


STORES = ('_frames', '_vviews', '_src_masks', '_intrinsics', '_poses', '_vposes', '_disp', '_flows', '_motion_mask', '_static_mask', '_flow_masks')


def assert_same_stores(a, b, names=STORES):
  for name in names:
    x, y = getattr(a, name, None), getattr(b, name, None)
    assert (x is None) == (y is None), name
    if x is not None:
      assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), name


def check_from_decoded(dev):
  import types
  from dynibar_amd import sample_ray
  from dynibar_amd.scene import DeviceScene
  dec = decoded_scene()
  a = DeviceScene.from_decoded(dev, batch=3, **dec)
  b = DeviceScene(dev, **host_prepared(dec))
  assert_same_stores(a, b)
  assert (a.N, a.H, a.W) == (b.N, b.H, b.W) == (7, 16, 23)
  args = types.SimpleNamespace(num_source_views=2, max_range=4, init_decay_epoch=10, num_vv=2, mask_src_view=False)
  batches = []
  for scene in (a, b):
    rng = np.random.RandomState(5)
    plan = scene.plan(0, args, rng=rng)
    sample_ray.rng.seed(7)
    batches.append(scene.sampler(plan).random_sample(64, 'uniform'))
  assert set(batches[0]) == set(batches[1])
  compared = 0
  for k, v in batches[0].items():
    if isinstance(v, torch.Tensor):
      assert torch.equal(v, batches[1][k]), k
      compared += 1
  assert compared >= 10


def check_constructors_take_device_tensors(dev):
  from dynibar_amd.scene import DeviceScene
  dec = decoded_scene(seed=1)
  hp = host_prepared(dec)
  big = ('images', 'disp', 'motion_mask', 'static_mask', 'flows', 'flow_masks', 'virtual_views')
  dp = {k: (dev_t(v, dev) if k in big else v) for k, v in hp.items()}
  assert_same_stores(DeviceScene(dev, **dp), DeviceScene(dev, **hp))
  rk = ('images', 'intrinsics', 'poses', 'depth_range', 'virtual_views', 'virtual_poses')
  src = np.where(mask01(7, 16, 23, seed=4) > 0, 255, 0).astype(np.uint8)
  assert_same_stores(DeviceScene.for_rendering(dev, source_masks=dev_t(src, dev), **{k: dp[k] for k in rk}),
                     DeviceScene.for_rendering(dev, source_masks=src, **{k: hp[k] for k in rk}))
  N, H, W = 12, 9, 11
  imgs, gtv = u8_image(N, H, W, 3, seed=6), u8_image(N, 12, H, W, 3, seed=7)
  gtm, cm = mask01(N, 12, H, W, seed=8).astype(F32), u8_image(N, H, W, seed=9)
  cams = np.tile(np.eye(4), (N, 1, 1))
  ea = DeviceScene.for_evaluation(dev, dev_t(imgs, dev), cams, cams, (F32(1), F32(20)), dev_t(cm, dev), dev_t(gtv, dev), dev_t(gtm, dev))
  eb = DeviceScene.for_evaluation(dev, imgs, cams, cams, (F32(1), F32(20)), cm, gtv, gtm)
  assert_same_stores(ea, eb, STORES + ('_gt_views', '_gt_masks'))
  assert ea.gt_mask_channels == eb.gt_mask_channels
  import pytest
  bad = dict(dp)
  bad['motion_mask'] = dp['motion_mask'] + 2
  with pytest.raises(ValueError, match='only 0 and 1'):
    DeviceScene(dev, **bad)
  bad = dict(dp)
  bad['disp'] = dp['disp'].double()
  with pytest.raises(ValueError, match='float32'):
    DeviceScene(dev, **bad)


def check_cli(dev, tmp_path, N=3, Hs=300, Ws=400):
  """python -m dynibar_amd.ingest on a small tree: the script's output tree, file names and array layouts, every value against the restatements"""
  import os
  from PIL import Image
  from dynibar_amd import ingest
  data_dir, cvd_dir = os.path.join(str(tmp_path), 'scene'), os.path.join(str(tmp_path), 'cvd')
  os.makedirs(os.path.join(data_dir, 'dense', 'images'))
  os.makedirs(cvd_dir)
  frames, depth = u8_image(N, Hs, Ws, 3, seed=21), f32_image(N, 60, 80, seed=21)
  rng = np.random.default_rng(21)
  c2w = np.tile(np.eye(4), (N, 1, 1))
  c2w[:, :3, :] = rng.standard_normal((N, 3, 4))
  K = np.array([[350.0, 0, 0], [0, 350.5, 0], [40, 30, 1]])  # stored transposed, for the 80 x 60 network input
  for i in range(N):
    Image.fromarray(frames[i]).save(os.path.join(data_dir, 'dense', 'images', '%05d.png' % i))
    np.savez(os.path.join(cvd_dir, 'batch%04d_out.npz' % i), img_1=np.zeros((1, 3, 60, 80), F32), depth=depth[i][None, None], K=K[None, None, None],
             cam_c2w=c2w[i][None])
  assert ingest.main(['--data_dir', data_dir, '--cvd_dir', cvd_dir, '--batch', '2']) == 0
  w, h = int(round(288 * (float(Ws) / float(Hs)))), 288
  dense = os.path.join(data_dir, 'dense')
  assert sorted(os.listdir(dense)) == sorted(['images', 'images_%dx%d' % (w, h), 'disp', 'poses_bounds_cvd.npy'])
  for i in range(N):
    img = np.asarray(Image.open(os.path.join(dense, 'images_%dx%d' % (w, h), '%05d.png' % i)))
    assert np.array_equal(img, resize_area(frames[i], (w, h))), i
    disp = np.load(os.path.join(dense, 'disp', '%05d.npy' % i))
    want = resize_linear(F32(1) / depth[i], (w, h))
    assert disp.dtype == F32 and np.array_equal(disp.view(np.uint32), want.view(np.uint32)), i
  rows = np.load(os.path.join(dense, 'poses_bounds_cvd.npy'))
  Ks = K.transpose().copy()
  Ks[0, :] *= w / 80
  Ks[1, :] *= h / 60
  want = ingest.poses_bounds(c2w, [depth_bounds(d) for d in depth], h, w, Ks[0, 0], Ks[1, 1])
  assert rows.shape == (N, 17) and rows.dtype == want.dtype and np.array_equal(rows, want)
