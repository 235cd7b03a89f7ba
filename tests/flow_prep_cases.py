"""Support for the flow-supervision tests (dynibar_amd/flow_prep.py, csrc/dyn_flowprep.h): seeded inputs, the numpy restatement of the contract in
include/dynibar_hip.h (flow supervision) and the checks the device and the emulator tests share.  Test infrastructure: nothing in dynibar_amd
imports this.

The restatement is written from the contract, not from the kernels.  numpy's float32 and float64 operations are single IEEE operations, which is
what "every product and sum is rounded on its own" asks for, so every device comparison is exact: np.array_equal on the bits, no tolerance.
tests/test_flow_prep_cpu.py pins the restatement itself to independent definitions."""
import functools

import numpy as np
import torch

from dynibar_amd import flow_prep  # (every test of this feature needs the module: none can pass without it)

F32 = np.float32
OFFSETS = (1, 2, 3, -1, -2, -3)
# (N, H, W): less than a wave, +-2 and +-3 never have a partner; +-3 in range for the end frames only; odd sizes; three tiles of the kernels'
# 4 rows x 64 pixels along each axis of the grid, the last one ragged in both
SCENE_SHAPES = [(2, 5, 7), (4, 9, 13), (7, 33, 31), (7, 11, 150)]
TILE_SHAPE = SCENE_SHAPES[3]
NONFINITE_FRAME = 1


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def axis(m, n, subpixel):
  """float32 coordinates along an axis of extent n -> (first tap int64, weight of the second tap float32)"""
  with np.errstate(all='ignore'):
    hi = F32(n + 1)
    m = np.where(m >= F32(-2), np.where(m <= hi, m, hi), F32(-2)).astype(F32)  # (NaN fails the first comparison)
    if subpixel:
      s = np.rint(m * F32(32)).astype(np.int64)
      return s >> 5, (s & 31).astype(F32) / F32(32)
    f = np.floor(m)
    return f.astype(np.int64), (m - f).astype(F32)


def warp_coordinates(flow):
  H, W = flow.shape[:2]
  return np.arange(W, dtype=F32)[None, :] + flow[:, :, 0], np.arange(H, dtype=F32)[:, None] + flow[:, :, 1]


def warp(img, flow, subpixel=32):
  """dyn_warp_flow for one image: float32 [H, W, C] sampled at pixel + flow, float32 [H, W, 2]"""
  assert img.dtype == F32 and flow.dtype == F32 and img.ndim == 3
  H, W = flow.shape[:2]
  mx, my = warp_coordinates(flow)
  ix, ax = axis(mx, W, subpixel)
  iy, ay = axis(my, H, subpixel)
  bx, by = F32(1) - ax, F32(1) - ay

  def tap(yy, xx):
    inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
    return np.where(inside[:, :, None], img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], F32(0))

  with np.errstate(all='ignore'):
    w = [(bx * by)[:, :, None], (ax * by)[:, :, None], (bx * ay)[:, :, None], (ax * ay)[:, :, None]]
    out = ((tap(iy, ix) * w[0] + tap(iy, ix + 1) * w[1]) + tap(iy + 1, ix) * w[2]) + tap(iy + 1, ix + 1) * w[3]
  assert out.dtype == F32
  return out


def consistency(f, w, alpha1=0.5, alpha2=0.5):
  """own flow f and warped partner flow w, float32 [H, W, 2] -> uint8 [H, W]"""
  f, w = f.astype(np.float64), w.astype(np.float64)
  with np.errstate(all='ignore'):
    a, b = f[..., 0] + w[..., 0], f[..., 1] + w[..., 1]
    e = np.sqrt(a * a + b * b)
    t = alpha1 * (np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + np.sqrt(w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1])) + alpha2
    return (e < t).astype(np.uint8)


def sampson(F, flow):
  """row-major F float64 [9] and the flow float32 [H, W, 2] of a frame pair -> float32 [H, W]"""
  H, W = flow.shape[:2]
  F = np.asarray(F, dtype=np.float64).reshape(3, 3)
  x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
  finite = np.isfinite(flow).all(axis=2)
  with np.errstate(all='ignore'):
    x2, y2 = x + flow[:, :, 0].astype(np.float64), y + flow[:, :, 1].astype(np.float64)
    l = [(F[k, 0] * x + F[k, 1] * y) + F[k, 2] for k in range(3)]
    m0 = (F[0, 0] * x2 + F[1, 0] * y2) + F[2, 0]
    m1 = (F[0, 1] * x2 + F[1, 1] * y2) + F[2, 1]
    r = (x2 * l[0] + y2 * l[1]) + l[2]
    den = ((l[0] * l[0] + l[1] * l[1]) + m0 * m0) + m1 * m1
    e = (np.abs(r) / np.sqrt(den)).astype(F32)
  return np.where(finite & (den > 0), e, F32(0)).astype(F32)


def supervision(flows, F=None, alpha1=0.5, alpha2=0.5, subpixel=32, epi_thresh=1.0, min_votes=2):
  """dyn_flow_supervision: flows float32 [N, 6, H, W, 2], F float64 [N, 6, 9] or None -> (masks uint8, epi float32 or None, motion uint8 or None)"""
  N, _, H, W, _ = flows.shape
  masks = np.zeros((N, 6, H, W), np.uint8)
  epi = np.zeros((N, 6, H, W), F32) if F is not None else None
  votes = np.zeros((N, H, W), np.int64)
  for i in range(N):
    for j, o in enumerate(OFFSETS):
      p = i + o
      if not 0 <= p < N:
        continue
      f = flows[i, j]
      masks[i, j] = consistency(f, warp(flows[p, (j + 3) % 6], f, subpixel), alpha1, alpha2)
      if F is not None:
        epi[i, j] = sampson(F[i, j], f)
        votes[i] += (masks[i, j] == 1) & (epi[i, j] > F32(epi_thresh))
  return masks, epi, ((votes >= min_votes).astype(np.uint8) if F is not None else None)


def in_range(N):
  """bool [N, 6]: the pairs whose partner frame is inside the scene"""
  return np.array([[0 <= i + o < N for o in OFFSETS] for i in range(N)])


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def smooth(rng, H, W, amplitude, channels=2):
  """a smooth random field [H, W, channels] within +-amplitude: three plane waves per channel, of periods of 5 pixels and more along each axis
  (short enough that a flow of 3 px and its negative, sampled 3 px apart, part ways on a good share of the pixels)"""
  y, x = np.mgrid[0:H, 0:W].astype(np.float64)
  out = np.zeros((H, W, channels))
  for c in range(channels):
    for _ in range(3):
      fx, fy = rng.uniform(-0.2, 0.2, 2)
      out[:, :, c] += np.sin(2 * np.pi * (fx * x + fy * y) + rng.uniform(0, 2 * np.pi))
  return out * (amplitude / 3.0)


@functools.lru_cache(maxsize=None)
def scene_flows(N, H, W, nonfinite=False, seed=0):
  """float32 [N, 6, H, W, 2], read-only: forward flows of amplitude 3 px, backward flows that are their approximate inverse plus smooth noise
  of amplitude 0.8 px, so that the consistency check passes on a part of every pair; the slots without a partner hold flow too (their outputs
  must be zero whatever they hold).  nonfinite: frame NONFINITE_FRAME also holds NaN, +-inf and 1e30."""
  rng = np.random.default_rng([seed, 21, N, H, W])
  flows = np.zeros((N, 6, H, W, 2), F32)
  for i in range(N):
    for j, o in enumerate(OFFSETS):
      if o > 0 or not 0 <= i + o < N:
        flows[i, j] = smooth(rng, H, W, 3.0)
  for i in range(N):
    for j, o in enumerate(OFFSETS):
      if o < 0 and 0 <= i + o < N:
        flows[i, j] = -flows[i + o, j - 3].astype(np.float64) + smooth(rng, H, W, 0.8)
  if nonfinite:
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], F32)
    for j in range(6):
      ys, xs = rng.integers(0, H, 6), rng.integers(0, W, 6)
      flows[NONFINITE_FRAME, j, ys, xs, rng.integers(0, 2, 6)] = bad[rng.integers(0, 5, 6)]
    flows[NONFINITE_FRAME, 0, 0, 0], flows[NONFINITE_FRAME, 3, H - 1, W - 1] = (np.nan, 1.0), (np.inf, -np.inf)
    flows[NONFINITE_FRAME, 0, H - 1, 0], flows[NONFINITE_FRAME, 3, 0, W - 1] = (1e30, 0.0), (0.5, -1e30)
  flows.setflags(write=False)
  return flows


@functools.lru_cache(maxsize=None)
def scene_cameras(N, H, W, seed=0):
  """(intrinsics float64 [N, 4, 4], camera-to-world float64 [N, 4, 4]): a camera that drifts and turns a little from frame to frame"""
  rng = np.random.default_rng([seed, 22, N, H, W])
  K = np.tile(np.eye(4), (N, 1, 1))
  K[:, 0, 0] = K[:, 1, 1] = 0.8 * W * rng.uniform(0.98, 1.02, N)
  K[:, 0, 2], K[:, 1, 2] = (W - 1) * 0.5, (H - 1) * 0.5
  c2w = np.tile(np.eye(4), (N, 1, 1))
  for i in range(N):
    c2w[i, :3, :3] = rotation(rng.uniform(-0.03, 0.03, 3))
    c2w[i, :3, 3] = np.array([0.1 * i, 0.02 * i, 0.01 * i]) + rng.uniform(-0.02, 0.02, 3)
  return K, c2w


def rotation(r):
  """Rodrigues: the rotation by |r| about r"""
  th = np.linalg.norm(r)
  if th == 0:
    return np.eye(3)
  k = r / th
  Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
  return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def static_scene_flow(H, W, seed=0):
  """A static scene seen by two cameras: (K [2, 4, 4], c2w [2, 4, 4], flows float32 [2, 6, H, W, 2] with slot 0 of frame 0 and slot 3 of frame 1
  the projections of a random depth map, computed in double and rounded to float32; |flow| < 64)."""
  rng = np.random.default_rng([seed, 23, H, W])
  K = np.tile(np.eye(4), (2, 1, 1))
  K[:, 0, 0] = K[:, 1, 1] = 0.9 * W
  K[:, 0, 2], K[:, 1, 2] = (W - 1) * 0.5, (H - 1) * 0.5
  c2w = np.tile(np.eye(4), (2, 1, 1))
  c2w[1, :3, :3] = rotation(np.array([0.01, -0.02, 0.005]))
  c2w[1, :3, 3] = (0.15, 0.03, 0.02)
  flows = np.zeros((2, 6, H, W, 2), F32)
  y, x = np.mgrid[0:H, 0:W].astype(np.float64)
  pix = np.stack([x, y, np.ones_like(x)], axis=-1)
  for a, b, slot in ((0, 1, 0), (1, 0, 3)):
    depth = 2.0 + 3.0 * rng.random((H, W)) + smooth(rng, H, W, 1.0, 1)[:, :, 0]
    cam = (pix @ np.linalg.inv(K[a, :3, :3]).T) * depth[:, :, None]
    world = cam @ c2w[a, :3, :3].T + c2w[a, :3, 3]
    w2c = np.linalg.inv(c2w[b])
    q = (world @ w2c[:3, :3].T + w2c[:3, 3]) @ K[b, :3, :3].T
    flow = q[:, :, :2] / q[:, :, 2:3] - pix[:, :, :2]
    assert np.abs(flow).max() < 64
    flows[a, slot] = flow
  return K, c2w, flows


# ---- shared device checks ------------------------------------------------------------------------------------------------------------
def dev_t(x, dev):
  return torch.from_numpy(np.array(x)).to(dev)  # (a copy: the shared inputs are read-only)


def host(t):
  return t.cpu().numpy()


def same_bits(got, want):
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
  view = {4: np.uint32, 1: np.uint8, 8: np.uint64}[got.dtype.itemsize]
  return np.array_equal(got.view(view), want.view(view))


@functools.lru_cache(maxsize=None)
def expected(N, H, W, subpixel, cameras, nonfinite=False):
  """the restatement's (masks, epi, motion, F) for scene_flows(N, H, W): computed once per session, shared and left unchanged"""
  flows = scene_flows(N, H, W, nonfinite)
  F = flow_prep.fundamental_matrices(*scene_cameras(N, H, W)) if cameras else None
  masks, epi, motion = supervision(flows, F, subpixel=subpixel)
  for a in (masks, epi, motion, F):
    if a is not None:
      a.setflags(write=False)
  return masks, epi, motion, F


def assert_both_mask_values(masks, N):
  """a comparison of all-zero (or all-one) masks shows nothing: both values make up at least 10 % of the in-range pixels"""
  live = masks[in_range(N)]
  ones = float(live.mean())
  assert 0.10 <= ones <= 0.90, f'{ones:.3f} of the in-range mask pixels are 1'
  return ones


def check_supervision(dev, N, H, W, subpixel, cameras, want_epi=True):
  flows = scene_flows(N, H, W)
  masks, epi, motion, _ = expected(N, H, W, subpixel, cameras)
  assert_both_mask_values(masks, N)
  d = dev_t(flows, dev)
  K, c2w = scene_cameras(N, H, W) if cameras else (None, None)
  got = flow_prep.supervision(d, K, c2w, subpixel=subpixel, want_epi=want_epi)
  assert set(got) == {'flow_masks'} | ({'motion'} if cameras else set()) | ({'epi'} if cameras and want_epi else set())
  assert got['flow_masks'].dtype == torch.uint8 and tuple(got['flow_masks'].shape) == (N, 6, H, W)
  assert same_bits(host(got['flow_masks']), masks), f'{int(np.sum(host(got["flow_masks"]) != masks))} mask bytes differ'
  assert not host(got['flow_masks'])[~in_range(N)].any(), 'a pair out of range wrote a mask'
  if cameras:
    assert same_bits(host(got['motion']), motion), f'{int(np.sum(host(got["motion"]) != motion))} motion bytes differ'
    if want_epi:
      assert same_bits(host(got['epi']), epi), f'{int(np.sum(host(got["epi"]).view(np.uint32) != epi.view(np.uint32)))} epi values differ'
      assert not host(got['epi'])[~in_range(N)].any(), 'a pair out of range wrote an epipolar error'
      assert float(epi.max()) > 1.0, 'the flows never leave their epipolar lines: the vote is not exercised'
  else:
    assert same_bits(host(flow_prep.consistency_masks(d, subpixel=subpixel)), masks)
  return got


def check_nonfinite(dev, N=4, H=9, W=13):
  """NaN, +-inf and 1e30 in one frame: mask 0 and epi 0 where the own flow is not finite, mask 0 for 1e30 (its warp leaves the image and
  e = |f| >= 0.5 |f| + 0.5), everything equal to the restatement and nothing out of range read (the clamp of fp_axis: read it as well)"""
  flows = scene_flows(N, H, W, True)
  for subpixel in (32, 0):
    masks, epi, motion, _ = expected(N, H, W, subpixel, True, True)
    K, c2w = scene_cameras(N, H, W)
    got = flow_prep.supervision(dev_t(flows, dev), K, c2w, subpixel=subpixel)
    assert same_bits(host(got['flow_masks']), masks) and same_bits(host(got['epi']), epi) and same_bits(host(got['motion']), motion)
    own = flows[NONFINITE_FRAME]
    nonfinite = ~np.isfinite(own).all(axis=-1)
    huge = np.abs(np.nan_to_num(own, nan=0.0, posinf=0.0, neginf=0.0)).max(axis=-1) >= 1e30
    assert nonfinite.sum() >= 4 and huge.sum() >= 2
    m, e = host(got['flow_masks'])[NONFINITE_FRAME], host(got['epi'])[NONFINITE_FRAME]
    assert not m[nonfinite].any() and not m[huge].any() and not e[nonfinite].any()
    assert np.isfinite(host(got['epi'])).all()


def check_prefilled_outputs_and_repeat(dev, N=4, H=9, W=13):
  """outputs prefilled with 0xFF / NaN come back complete; a second run, and a run on a side stream, give the same bits"""
  from dynibar_amd import _lib
  masks, epi, motion, F = expected(N, H, W, 32, True)
  d, Fd = dev_t(scene_flows(N, H, W), dev), dev_t(F, dev)

  def run():
    m = torch.full((N, 6, H, W), 0xFF, dtype=torch.uint8, device=dev)
    e = torch.full((N, 6, H, W), float('nan'), dtype=torch.float32, device=dev)
    v = torch.full((N, H, W), 0xFF, dtype=torch.uint8, device=dev)
    _lib.call('dyn_flow_supervision', N, H, W, d.data_ptr(), Fd.data_ptr(), 0.5, 0.5, 32, 1.0, 2, m.data_ptr(), e.data_ptr(), v.data_ptr(),
              _lib.stream_of(d))
    return m, e, v

  first, second = run(), run()
  for got, want in zip(first, (masks, epi, motion)):
    assert same_bits(host(got), want)
  for a, b in zip(first, second):
    assert same_bits(host(a), host(b))
  if torch.device(dev).type == 'cuda':
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      third = run()
    side.synchronize()
    for a, b in zip(first, third):
      assert same_bits(host(a), host(b))


def check_resize(dev, Hs, Ws, Hd, Wd, B=None, seed=0):
  """resize_flow against the existing linear resize on each channel plane times the stated fp32 ratio"""
  from dynibar_amd import ingest
  rng = np.random.default_rng([seed, 24, Hs, Ws, Hd, Wd])
  raw = (8.0 * rng.standard_normal(((B or 1), Hs, Ws, 2))).astype(F32)
  d = dev_t(raw if B else raw[0], dev)
  got = flow_prep.resize_flow(d, (Wd, Hd))
  assert got.dtype == torch.float32 and tuple(got.shape) == ((B, Hd, Wd, 2) if B else (Hd, Wd, 2))
  ratio = (F32(Wd / Ws), F32(Hd / Hs))
  for b in range(B or 1):
    for c in range(2):
      plane = host(ingest.resize_linear(dev_t(raw[b, :, :, c], dev), (Wd, Hd)))
      want = plane * ratio[c]
      assert want.dtype == F32
      assert same_bits(host(got[b] if B else got)[:, :, c], want), (b, c)
  if (Hs, Ws) == (Hd, Wd):
    assert same_bits(host(got), raw if B else raw[0])
  out = torch.full_like(got, float('nan'))
  assert flow_prep.resize_flow(d, (Wd, Hd), out=out) is out and same_bits(host(out), host(got))


def check_warp(dev, H=9, W=13):
  """C = 1, 3, 4, the batched and the unbatched forms, both coordinate modes, flows that leave the image on every side"""
  rng = np.random.default_rng([25, H, W])
  flow = (smooth(rng, H, W, 3.0) + rng.uniform(-0.5, 0.5, (H, W, 2))).astype(F32)
  flow[0, 0], flow[H - 1, W - 1], flow[0, W - 1], flow[H - 1, 0] = (-1.5, -0.25), (1.25, 0.75), (0.5, -2.5), (-30.0, 40.0)
  for subpixel in (32, 0):
    for C in (1, 3, 4):
      img = rng.standard_normal((H, W, C)).astype(F32)
      want = warp(img, flow, subpixel)
      got = flow_prep.warp_flow(dev_t(img, dev), dev_t(flow, dev), subpixel=subpixel)
      assert got.dtype == torch.float32 and tuple(got.shape) == (H, W, C)
      assert same_bits(host(got), want), (subpixel, C)
      if C == 1:  # [H, W], from host arrays
        assert same_bits(host(flow_prep.warp_flow(img[:, :, 0], flow, subpixel=subpixel, device=dev)), want[:, :, 0])
    imgs, flows = rng.standard_normal((2, H, W, 3)).astype(F32), np.stack([flow, flow[::-1, ::-1].copy()])
    got = flow_prep.warp_flow(dev_t(imgs, dev), dev_t(flows, dev), subpixel=subpixel)
    assert same_bits(host(got), np.stack([warp(imgs[b], flows[b], subpixel) for b in range(2)]))
    got = flow_prep.warp_flow(dev_t(imgs[:, :, :, 0], dev), dev_t(flows, dev), subpixel=subpixel)  # [B, H, W]
    assert same_bits(host(got), np.stack([warp(imgs[b, :, :, :1], flows[b], subpixel)[:, :, 0] for b in range(2)]))


def check_scene_takes_the_masks(dev, H=9, W=13):
  """supervision(...)['flow_masks'] goes into the DeviceScene constructor as it is, at the scene's minimum of 7 frames"""
  import scene_cases as sc
  from dynibar_amd import scene
  N = 7
  a = sc.make_scene(H, W, 0, N)
  flows = dev_t(scene_flows(N, H, W), dev)
  masks = flow_prep.supervision(flows)['flow_masks']
  s = scene.DeviceScene(dev, a['images'], a['intrinsics'], a['poses'], a['depth_range'], a['disp'], a['motion_mask'], a['static_mask'], flows, masks,
                        a['virtual_views'], a['virtual_poses'], a['source_masks'])
  assert s._flow_masks.dtype == torch.uint8 and same_bits(host(s._flow_masks), expected(N, H, W, 32, False)[0])
  if torch.device(dev).type == 'cuda':
    assert s._flow_masks.data_ptr() == masks.data_ptr() and s._flows.data_ptr() == flows.data_ptr(), 'the stores were copied'


def check_refusals(dev):
  import pytest
  from dynibar_amd import _lib
  N, H, W = 2, 5, 7
  flows = dev_t(scene_flows(N, H, W), dev)
  K, c2w = scene_cameras(N, H, W)
  for bad in (flows[:, :5], flows[..., :1], flows[0], flows[:0], flows.double()):  # wrong shapes, N = 0, a wrong dtype
    with pytest.raises(ValueError):
      flow_prep.supervision(bad)
    with pytest.raises(ValueError):
      flow_prep.consistency_masks(bad)
  with pytest.raises(ValueError, match='subpixel'):
    flow_prep.consistency_masks(flows, subpixel=16)
  with pytest.raises(ValueError, match='both intrinsics and poses'):
    flow_prep.supervision(flows, intrinsics=K)
  with pytest.raises(ValueError):
    flow_prep.supervision(flows, K[:1], c2w[:1])  # cameras of another scene
  with pytest.raises(ValueError):
    flow_prep.fundamental_matrices(K, c2w[:, :3])
  img = dev_t(np.zeros((H, W, 5), F32), dev)
  with pytest.raises(ValueError, match='1 to 4 channels'):
    flow_prep.warp_flow(img, flows[0, 0])
  with pytest.raises(ValueError):
    flow_prep.warp_flow(img[:, :, :3], flows[0, 0, :4])
  with pytest.raises(ValueError):
    flow_prep.warp_flow(img[:, :, :3], flows[0, 0], subpixel=1)
  with pytest.raises(ValueError):
    flow_prep.resize_flow(flows[0, 0], (0, 3))
  with pytest.raises(ValueError):
    flow_prep.resize_flow(flows[0, 0, :, :, 0], (4, 3))
  # the C entry refuses by itself, with a message: motion or epi without cameras, no frames, a channel count out of range
  m = torch.zeros((N, 6, H, W), dtype=torch.uint8, device=dev)
  v = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
  st = _lib.stream_of(flows)
  with pytest.raises(RuntimeError, match='need the fundamental matrices'):
    _lib.call('dyn_flow_supervision', N, H, W, flows.data_ptr(), None, 0.5, 0.5, 32, 1.0, 2, m.data_ptr(), None, v.data_ptr(), st)
  with pytest.raises(RuntimeError, match='N=0'):
    _lib.call('dyn_flow_supervision', 0, H, W, flows.data_ptr(), None, 0.5, 0.5, 32, 1.0, 2, m.data_ptr(), None, None, st)
  with pytest.raises(RuntimeError, match='unsupported'):
    _lib.call('dyn_flow_supervision', N, 65536, 32768, flows.data_ptr(), None, 0.5, 0.5, 32, 1.0, 2, m.data_ptr(), None, None, st)
  with pytest.raises(RuntimeError, match='C=5'):
    _lib.call('dyn_warp_flow', 1, H, W, 5, img.data_ptr(), flows.data_ptr(), m.data_ptr(), 32, st)
  with pytest.raises(RuntimeError, match='must differ'):
    _lib.call('dyn_flow_resize', 1, H, W, H, W, flows.data_ptr(), flows.data_ptr(), st)
  assert not host(m).any() and not host(v).any(), 'a refused call wrote'


def write_raw_tree(root, flows):
  """flow_i{1,2,3}/%05d_{fwd,bwd}.npz with the key flow, for the pairs in range only: what a flow network leaves"""
  import os
  N = flows.shape[0]
  for k in (1, 2, 3):
    os.makedirs(os.path.join(root, 'flow_i%d' % k), exist_ok=True)
  for i in range(N):
    for j, o in enumerate(OFFSETS):
      if 0 <= i + o < N:
        np.savez(os.path.join(root, 'flow_i%d' % abs(o), '%05d_%s.npz' % (i, 'fwd' if o > 0 else 'bwd')), flow=flows[i, j])


def check_cli(dev, tmp_path, N=4, H=9, W=13):
  """python -m dynibar_amd.flow_prep on a four-frame tree: the files have the loader's keys, shapes and dtypes, their mask is
  consistency_masks of their flow, out-of-range pairs have no file; then the same with a resize and cameras"""
  import os
  from PIL import Image
  raw, out = os.path.join(str(tmp_path), 'raw'), os.path.join(str(tmp_path), 'out')
  flows = scene_flows(N, H, W)
  write_raw_tree(raw, flows)
  assert flow_prep.main(['--raw_dir', raw, '--out_dir', out]) == 0

  def read_back(root, h, w):
    back = np.zeros((N, 6, h, w, 2), F32)
    masks = np.zeros((N, 6, h, w), np.uint8)
    for i in range(N):
      for j, o in enumerate(OFFSETS):
        path = os.path.join(root, 'flow_i%d' % abs(o), '%05d_%s.npz' % (i, 'fwd' if o > 0 else 'bwd'))
        assert os.path.exists(path) == (0 <= i + o < N), path
        if os.path.exists(path):
          z = np.load(path)
          assert sorted(z.files) == ['flow', 'mask']
          assert z['flow'].dtype == F32 and z['flow'].shape == (h, w, 2) and z['mask'].dtype == np.bool_ and z['mask'].shape == (h, w)
          back[i, j], masks[i, j] = z['flow'], z['mask']
    return back, masks

  back, masks = read_back(out, H, W)
  assert same_bits(back, np.where(in_range(N)[:, :, None, None, None], flows, F32(0)))
  assert same_bits(masks, host(flow_prep.consistency_masks(dev_t(back, dev))))
  assert same_bits(masks, expected(N, H, W, 32, False)[0])
  # with --size and --poses
  K, c2w = scene_cameras(N, H, W)
  h2, w2 = 11, 17
  llff = np.zeros((N, 3, 5))
  llff[:, :, 1], llff[:, :, 0], llff[:, :, 2], llff[:, :, 3] = c2w[:, :3, 0], c2w[:, :3, 1], -c2w[:, :3, 2], c2w[:, :3, 3]  # (x, -y, -z) stored as (-y, x, z)
  llff[:, :, 4] = (H, W, K[0, 0, 0])
  poses_path = os.path.join(str(tmp_path), 'poses_bounds.npy')
  np.save(poses_path, np.concatenate([llff.reshape(N, 15), np.ones((N, 2))], axis=1))
  Kr, cr = flow_prep.read_cameras(poses_path, (w2, h2))
  assert np.allclose(cr, c2w, atol=1e-12) and np.allclose(Kr[:, 0, 0], K[0, 0, 0] * w2 / W) and np.allclose(Kr[:, 0, 2], w2 / 2.0)
  out2 = os.path.join(str(tmp_path), 'out2')
  assert flow_prep.main(['--raw_dir', raw, '--out_dir', out2, '--size', str(w2), str(h2), '--poses', poses_path, '--epi_thresh', '0.5']) == 0
  back2, masks2 = read_back(out2, h2, w2)
  res = flow_prep.supervision(dev_t(back2, dev), Kr, cr, epi_thresh=0.5)
  assert same_bits(masks2, host(res['flow_masks']))
  for i in range(N):
    png = np.asarray(Image.open(os.path.join(out2, 'flow_motion_masks', '%d.png' % i)))
    assert png.dtype == np.uint8 and same_bits(png, host(res['motion'])[i] * np.uint8(255))
