"""Support for the view-log tests (dynibar_amd/view_log.py, csrc/dyn_viewlog.h): seeded inputs, numpy restatements of what the training loop's
logging branch computes on the host (train.py:657-759 log_view_to_tb; utils.py:97-170 colorize / colorize_np; ibrnet/data_loaders/flow_utils.py:17-153
make_color_wheel / compute_color / flow_to_image), and the checks the device and the emulator tests share.  Test infrastructure: nothing in
dynibar_amd imports this.

The restatements are compared with the real functions' outputs in tests/golden/view_log.npz (tests/test_view_log_cpu.py: exact), and the kernels
with the restatements (exact).  They run on numpy >= 2: a float64 numpy scalar keeps its precision against a float32 array there, which is what
makes the normalisation of colorize and everything after flow_to_image's divisor float64."""
import functools
import os
from collections import OrderedDict

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'view_log.npz')
MAPS = ('jet', 'gray')
SCALAR_DATA = ('uniform', 'heavy_tail', 'all_equal', 'few_values', 'signs_zeros_denormals', 'last_ten_bits')
FLOW_CASES = ('scale0.3', 'scale3', 'scale30', 'scale120_unknown', 'zero', 'axis', 'unknown_largest')
SHAPES = [(1, 1), (1, 2), (7, 9), (8, 8), (5, 13), (33, 31), (25, 41), (48, 80), (97, 131)]
FLOW_SHAPES = SHAPES[:-1]
GOLDEN_SHAPES = [(7, 9), (33, 31), (48, 80)]  # the cases the fixture holds: every data set / flow case at these shapes
PLAN_SIZES = (1, 2, 3, 64, 65, 101, 3840, 147456)


@functools.lru_cache(maxsize=1)
def golden():
  with np.load(GOLDEN) as z:
    return {k: z[k] for k in z.files}


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _name_id(name, names):
  return names.index(name)


def scalar_data(name, H, W, fresh=False):
  """float32 [H, W], finite; a fixture case is read from the fixture (the bits do not depend on this numpy's generator then)"""
  key = f'colorize/{name}/{H}x{W}/x'
  if not fresh and (H, W) in GOLDEN_SHAPES and os.path.exists(GOLDEN) and key in golden():
    return golden()[key].copy()
  rng = np.random.default_rng([_name_id(name, SCALAR_DATA), H, W, 20])
  n = H * W
  if name == 'uniform':
    x = rng.random(n) * 7.0 + 0.5
  elif name == 'heavy_tail':
    x = rng.standard_normal(n) ** 3 * 10.0
  elif name == 'all_equal':  # vmin == p99, the range is exactly 1e-6
    x = np.full(n, 0.37)
  elif name == 'few_values':  # fewer than ten distinct values: both percentile ranks fall inside runs of ties
    x = rng.choice(np.array([-2.0, -0.5, 0.25, 0.75, 1.0, 3.5, 8.0]), n)
  elif name == 'signs_zeros_denormals':
    pool = np.array([-1.5, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, -3e-39, 2.5, -1e-3, 1e-3, 7e-39], dtype=np.float32)
    x = np.where(rng.random(n) < 0.7, rng.choice(pool, n), rng.standard_normal(n).astype(np.float32) * np.float32(1e-2))
  elif name == 'last_ten_bits':  # keys that differ only in the last 10 bits: the third radix pass decides
    x = (np.uint32(0x3FC00000) | rng.integers(0, 1024, n).astype(np.uint32)).view(np.float32)
  else:
    raise KeyError(name)
  return np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(H, W))


def flow_data(case, H, W, fresh=False):
  """float32 [H, W, 2], finite"""
  key = f'flow/{case}/{H}x{W}/flow'
  if not fresh and (H, W) in GOLDEN_SHAPES and os.path.exists(GOLDEN) and key in golden():
    return golden()[key].copy()
  rng = np.random.default_rng([_name_id(case, FLOW_CASES), H, W, 21])
  n = H * W
  if case.startswith('scale'):
    f = rng.standard_normal((n, 2)) * float(case[5:].split('_')[0])
    if case.endswith('unknown'):  # |u| or |v| above 200 here and there, next to what the scale itself throws above it
      hit = rng.random(n) < 0.1
      f[hit, rng.integers(0, 2, int(hit.sum()))] = rng.choice(np.array([200.5, -250.0, 1e4, -201.0]), int(hit.sum()))
      f[0] = (200.0, -200.0)  # exactly the threshold: known
  elif case == 'zero':  # the divisor is eps and every pixel white
    f = np.zeros((n, 2))
  elif case == 'axis':  # both ends of the angle, the k1 == 56 -> 1 wrap, the rad <= 1 boundary at the largest radius
    pool = np.array([(1, 0), (-1, 0), (0, 1), (0, -1), (-1, -0.0), (1, -0.0), (-0.0, 1), (0.5, 0), (0, -0.25), (0, 0), (-0.0, -0.0)], dtype=np.float32)
    f = pool[np.arange(n) % len(pool)]
  elif case == 'unknown_largest':  # one unknown pixel that would have been the largest radius
    f = rng.standard_normal((n, 2)) * 3.0
    f[n // 2] = (150.0, 201.0)
  else:
    raise KeyError(case)
  return np.ascontiguousarray(np.asarray(f, dtype=np.float32).reshape(H, W, 2))


def vector_data(n, seed=5):
  """float32 [n, 3] for the magnitude: several scales, zeros, a denormal and a huge row"""
  rng = np.random.default_rng([seed, n, 22])
  v = (rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-3, 3, (n, 1))).astype(np.float32)
  v[:: 17, 1] = 0.0
  v[0] = 0.0
  if n > 2:
    v[1] = (1e-30, -2e-30, 1e-39)
    v[2] = (3e18, -1e18, 2e18)
  return v


# ---- restatements ------------------------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
  """float32 fma of arrays without a fused instruction: the product of two float32 is exact in float64; the float64 sum is rounded TO ODD (the
  error term of TwoSum says whether it was inexact and on which side), after which the rounding to float32 is the single rounding of fmaf."""
  a, b, c = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (a, b, c))
  p = a * b
  s = p + c
  bb = s - p
  err = (p - (s - bb)) + (c - bb)
  even = (s.view(np.int64) & 1) == 0
  fix = (err != 0) & even & np.isfinite(s)
  s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
  return s.astype(np.float32)


def magnitude(v):
  """torch.norm(v, dim=-1) on the host (train.py:674): sqrtf(fmaf(z, z, fmaf(y, y, x * x)))"""
  v = np.asarray(v, dtype=np.float32)
  x, y, z = v[..., 0], v[..., 1], v[..., 2]
  return np.sqrt(fmaf(z, z, fmaf(y, y, x * x)))


def lerp_from_plan(x, rank, weight):
  """(p1, p99) from the sorted values by numpy's _lerp, the way k_viewlog_ranges forms them from the plan of view_log.percentile_plan"""
  s = np.sort(np.asarray(x, dtype=np.float32).reshape(-1))
  out = []
  for q in range(2):
    a, b = s[rank[2 * q]], s[rank[2 * q + 1]]
    d = np.float32(b - a)
    t = np.float64(weight[q])
    out.append(np.float64(b) - np.float64(d) * (1 - t) if t >= 0.5 else np.float64(a) + np.float64(d) * t)
  return np.array(out, dtype=np.float64)


def ranges_restated(x):
  """utils.py:117-118"""
  vmin, vmax = np.percentile(x, (1, 99))
  vmax += 1e-6
  return np.float64(vmin), np.float64(vmax)


def colorize_restated(x, cmap_name):
  """colorize_np without mask, range and colour bar (utils.py:117-125), matplotlib's Colormap.__call__ on a float array written out:
  index = int(x * N), x == 1 -> N - 1, into the N = 256 rows of the map's table -> float64 [H, W, 3]"""
  from dynibar_amd import view_log
  x = np.asarray(x)
  assert x.dtype == np.float32
  vmin, vmax = ranges_restated(x)
  y = np.clip(x, vmin, vmax)
  y = (y - vmin) / (vmax - vmin)
  y = np.clip(y, 0.0, 1.0)
  assert y.dtype == np.float64, 'numpy < 2 normalises in float32: the contract is numpy >= 2'
  idx = np.minimum((y * 256).astype(int), 255)
  return view_log.table(cmap_name).numpy()[idx]


def color_wheel():
  """make_color_wheel (flow_utils.py:17-64): 55 rows"""
  rows = []
  for count, fixed, ramp, down in ((15, 0, 1, False), (6, 1, 0, True), (4, 1, 2, False), (11, 2, 1, True), (13, 2, 0, False), (6, 0, 2, True)):
    for i in range(count):
      row = [0.0, 0.0, 0.0]
      row[fixed] = 255.0
      step = np.floor(255 * i / count)
      row[ramp] = 255.0 - step if down else step
      rows.append(row)
  return np.array(rows)


def flow_to_image_restated(flow):
  """flow_to_image with compute_color (flow_utils.py:67-153) on a COPY of flow -> uint8 [H, W, 3]"""
  flow = np.array(flow, dtype=np.float32, copy=True)
  u, v = flow[:, :, 0], flow[:, :, 1]
  unknown = (abs(u) > 200) | (abs(v) > 200)
  u[unknown] = 0
  v[unknown] = 0
  rad = np.sqrt(u ** 2 + v ** 2)
  maxrad = max(-1, np.max(rad))
  u = u / (maxrad + np.finfo(float).eps)
  v = v / (maxrad + np.finfo(float).eps)
  assert u.dtype == np.float64, 'numpy < 2 divides in float32: the contract is numpy >= 2'
  wheel = color_wheel()
  ncols = wheel.shape[0]
  rad = np.sqrt(u ** 2 + v ** 2)
  a = np.arctan2(-v, -u) / np.pi
  fk = (a + 1) / 2 * (ncols - 1) + 1
  k0 = np.floor(fk).astype(int)
  k1 = k0 + 1
  k1[k1 == ncols + 1] = 1
  f = fk - k0
  img = np.zeros(u.shape + (3,))
  for i in range(3):
    col0 = wheel[:, i][k0 - 1] / 255
    col1 = wheel[:, i][k1 - 1] / 255
    col = (1 - f) * col0 + f * col1
    idx = rad <= 1
    col[idx] = 1 - rad[idx] * (1 - col[idx])
    col[~idx] *= 0.75
    img[:, :, i] = np.uint8(np.floor(255 * col))
  img[unknown] = 0
  return np.uint8(img)


def flow_angles(flow):
  """the double angle atan2(-v, -u) per pixel, for the report of a differing byte"""
  flow = np.array(flow, dtype=np.float32, copy=True)
  u, v = flow[:, :, 0], flow[:, :, 1]
  unknown = (abs(u) > 200) | (abs(v) > 200)
  u[unknown] = 0
  v[unknown] = 0
  d = np.max(np.sqrt(u ** 2 + v ** 2)) + np.finfo(float).eps
  return np.arctan2(-(v / d), -(u / d))


def hwc2chw(t):
  return t.permute(2, 0, 1)


def panels_restated(ret, gt_img, gt_disp, gt_flows):
  """train.py:657-759 on host tensors -> OrderedDict tag -> what the writer is handed"""
  ref, st, anchor = ret['outputs_coarse_ref'], ret['outputs_coarse_st'], ret['outputs_coarse_anchor']
  out = OrderedDict()
  for tag, t in (('render_rgb_coarse_ref', ref['rgb']), ('render_rgb_coarse_anchor', anchor['rgb']), ('render_rgb_static', ref['rgb_static']),
                 ('render_rgb_dynamic', ref['rgb_dy']), ('st_rgb_pred', st['rgb'])):
    out[tag] = torch.clamp(hwc2chw(t), 0.0, 1.0)
  exp_sf_mag = torch.norm(ref['exp_sf'], dim=-1)
  for tag, x, name in (('render_depth_coarse', ref['depth'], 'jet'), ('occ_weight_map', anchor['occ_weight_map'], 'gray'),
                       ('exp_sf_mag', exp_sf_mag, 'gray'), ('gt_disp_coarse', gt_disp[..., 0], 'jet')):
    out[tag] = hwc2chw(torch.from_numpy(colorize_restated(x.numpy(), name)))
  out['gt_rgb_coarse'] = hwc2chw(gt_img)
  H, W = gt_img.shape[0], gt_img.shape[1]
  gt_flows = gt_flows.reshape(gt_flows.shape[0], H, W, 2)
  n = min(6, gt_flows.shape[0])
  out['rd_flow_stack'] = torch.stack([torch.Tensor(flow_to_image_restated(ref['render_flows'][i].numpy()) / 255.0) for i in range(n)], dim=0)
  out['gt_flow_stack'] = torch.stack([torch.Tensor(flow_to_image_restated(gt_flows[i].numpy()) / 255.0) for i in range(n)], dim=0)
  return out


# ---- shared checks (device: a HIP device, or 'cpu' under the emulator) ------------------------------------------------------------------
def _dev(a, device):
  return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def assert_same(got, want, what):
  """exact: shape, dtype and every value (torch.equal)"""
  got = got.cpu() if isinstance(got, torch.Tensor) else torch.from_numpy(np.asarray(got))
  want = want if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
  assert tuple(got.shape) == tuple(want.shape), f'{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}'
  assert got.dtype == want.dtype, f'{what}: dtype {got.dtype} vs {want.dtype}'
  if not torch.equal(got, want):
    bad = (got != want).nonzero()
    i = tuple(int(v) for v in bad[0])
    raise AssertionError(f'{what}: {bad.shape[0]} of {got.numel()} values differ, first at {i}: {got[i].item()!r} vs {want[i].item()!r}')


def check_ranges_and_colorize(device, H, W, name):
  """the ranges of one image alone and of four in one call (the third in the magnitude form) against np.percentile, the magnitude against the
  fma chain and torch.norm, colorize with both maps against the restatement and, for a fixture case, the real function's output"""
  from dynibar_amd import view_log
  x = scalar_data(name, H, W)
  others = [scalar_data(SCALAR_DATA[(SCALAR_DATA.index(name) + k) % len(SCALAR_DATA)], H, W) for k in (1, 2)]
  vec = vector_data(H * W, seed=H + W).reshape(H, W, 3)
  mag = magnitude(vec)
  assert np.array_equal(mag, torch.norm(torch.from_numpy(vec), dim=-1).numpy())
  xd, vd = _dev(x, device), _dev(vec, device)
  before = xd.clone(), vd.clone()
  alone, (img,) = view_log.ranges([xd])
  assert img.data_ptr() == xd.data_ptr()
  assert_same(alone, np.array([ranges_restated(x)]), f'ranges of {name} {H}x{W} alone')
  four, imgs = view_log.ranges([_dev(others[0], device), xd, vd, _dev(others[1], device)])
  assert_same(four, np.array([ranges_restated(others[0]), ranges_restated(x), ranges_restated(mag), ranges_restated(others[1])]),
              f'ranges of {name} {H}x{W}, four images in one call')
  assert_same(imgs[2], mag, 'the magnitude image')
  g = golden() if (H, W) in GOLDEN_SHAPES else {}
  for cmap in MAPS:
    got = view_log.colorize(xd, cmap)
    assert_same(got, colorize_restated(x, cmap), f'colorize({name} {H}x{W}, {cmap})')
    if f'colorize/{name}/{H}x{W}/{cmap}' in g:
      assert_same(got, g[f'colorize/{name}/{H}x{W}/{cmap}'], f'colorize({name} {H}x{W}, {cmap}) against the real function')
  assert torch.equal(before[0], xd) and torch.equal(before[1], vd), 'an input was written'


def check_flow(device, H, W, case):
  """flow_to_image against the restatement (and the real function's output for a fixture case); maxrad; the input is unchanged"""
  from dynibar_amd import view_log
  f = flow_data(case, H, W)
  fd = _dev(f, device)
  before = fd.clone()
  known = np.where(((abs(f[..., 0]) > 200) | (abs(f[..., 1]) > 200))[..., None], np.float32(0), f)
  want_max = np.float32(max(-1, np.max(np.sqrt(known[..., 0] ** 2 + known[..., 1] ** 2))))
  assert_same(view_log.flow_max([fd]), np.array([want_max]), f'maxrad of {case} {H}x{W}')
  got = view_log.flow_to_image(fd)
  want = flow_to_image_restated(f)
  report_flow_bytes(got, want, f, f'flow_to_image({case} {H}x{W})')
  g = golden() if (H, W) in GOLDEN_SHAPES else {}
  if f'flow/{case}/{H}x{W}/img' in g:
    report_flow_bytes(got, g[f'flow/{case}/{H}x{W}/img'], f, f'flow_to_image({case} {H}x{W}) against the real function')
  if case == 'zero':
    assert bool((got == 255).all())
  assert torch.equal(before, fd), 'the flow was written'


def report_flow_bytes(got, want, flow, what):
  """exact; a differing byte is reported with its pixel and the host's angle there (the two libraries' double atan2 may differ in the last bit,
  which moves a byte only for a pixel on a floor boundary: no tolerance)"""
  got = got.cpu().numpy()
  assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, f'{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}'
  if not np.array_equal(got, want):
    ang = flow_angles(flow)
    bad = np.argwhere(got != want)
    lines = [f'pixel ({y}, {x}) channel {c}: {got[y, x, c]} vs {want[y, x, c]}, flow {flow[y, x].tolist()}, host angle {float(ang[y, x])!r} '
             f'({float(ang[y, x]).hex()})' for y, x, c in bad[:8]]
    raise AssertionError(f'{what}: {len(bad)} bytes differ\n' + '\n'.join(lines))


def synthetic_groups(H, W, n_flows, seed=3):
  """host tensors shaped like a render_single_image_mono result in 'device' mode and the frame's ground truth"""
  rng = np.random.default_rng([seed, H, W, n_flows])
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))
  rgb = lambda: t(rng.random((H, W, 3)) * 1.4 - 0.2)
  ref = OrderedDict(rgb=rgb(), rgb_static=rgb(), rgb_dy=rgb(), depth=t(1.0 + 19.0 * rng.random((H, W)) ** 2), exp_sf=t(rng.standard_normal((H, W, 3)) * 0.1),
                    render_flows=t(rng.standard_normal((n_flows, H, W, 2)) * 5.0))
  ref['rgb'][0, 0] = torch.tensor([-0.0, 1.0, 0.0])
  ref['render_flows'][0, H // 2, W // 2] = torch.tensor([300.0, 1.0])
  st = OrderedDict(rgb=rgb())
  anchor = OrderedDict(rgb=rgb(), occ_weight_map=t(rng.random((H, W))))
  ret = OrderedDict(outputs_coarse_ref=ref, outputs_coarse_st=st, outputs_coarse_anchor=anchor)
  gt_flows = t(rng.standard_normal((n_flows, H * W, 2)) * 40.0)
  return ret, t(rng.random((H, W, 3))), t(0.05 + rng.random((H, W, 1))), gt_flows


class StubWriter(object):
  """records what a SummaryWriter would be handed"""

  def __init__(self):
    self.calls = []

  def add_image(self, tag, img_tensor, global_step=None, walltime=None, dataformats='CHW'):
    self.calls.append(('add_image', tag, img_tensor, global_step, dataformats))

  def add_images(self, tag, img_tensor, global_step=None, walltime=None, dataformats='NCHW'):
    self.calls.append(('add_images', tag, img_tensor, global_step, dataformats))


def to_device(ret, device):
  return OrderedDict((g, OrderedDict((k, v.to(device)) for k, v in grp.items())) for g, grp in ret.items())


def check_panel_values(got, want, n_flows, H, W):
  from dynibar_amd import view_log
  assert list(got.keys()) == list(want.keys()) == list(view_log.TAGS)
  n = min(6, n_flows)
  for tag in view_log.TAGS:
    assert_same(got[tag], want[tag].contiguous(), tag)
    shape = (n, H, W, 3) if tag.endswith('_stack') else (3, H, W)
    dtype = torch.float64 if tag in view_log.MAP_TAGS else torch.float32
    assert tuple(got[tag].shape) == shape and got[tag].dtype == dtype, f'{tag}: {tuple(got[tag].shape)} {got[tag].dtype}'


def check_panels(device, H, W, n_flows):
  """every tag's shape, dtype and bits against the restatement on host copies; the inputs are unchanged; .cpu() equals the device views; the stub
  writer receives the reference's twelve calls in its order"""
  from dynibar_amd import view_log
  ret, gt_img, gt_disp, gt_flows = synthetic_groups(H, W, n_flows)
  want = panels_restated(ret, gt_img, gt_disp, gt_flows)
  dret = to_device(ret, device)
  dgt = gt_img.to(device), gt_disp.to(device), gt_flows.to(device)
  got = view_log.panels(dret, *dgt)
  check_panel_values(got, want, n_flows, H, W)
  for g, grp in ret.items():
    for k, v in grp.items():
      assert torch.equal(dret[g][k].cpu(), v), f'{g}/{k} was written'
  for a, b in zip(dgt, (gt_img, gt_disp, gt_flows)):
    assert torch.equal(a.cpu(), b), 'the ground truth was written'
  host = got.cpu()
  assert list(host.keys()) == list(got.keys())
  for tag in got:
    assert host[tag].device.type == 'cpu' and torch.equal(host[tag], got[tag].cpu()) and host[tag].dtype == got[tag].dtype
  lo = host.buffer.data_ptr()
  assert all(lo <= t.data_ptr() < lo + host.buffer.numel() for t in host.values()), 'the host panels are views into one buffer'
  w = StubWriter()
  got.write(w, 1234, 'train/')
  assert [c[0] for c in w.calls] == ['add_image'] * 10 + ['add_images'] * 2
  assert [c[1] for c in w.calls] == ['train/' + t for t in view_log.TAGS]
  assert [c[4] for c in w.calls] == ['CHW'] * 10 + ['NHWC'] * 2 and all(c[3] == 1234 for c in w.calls)
  for c in w.calls:
    assert c[2].device.type == 'cpu'
    assert_same(c[2], want[c[1][len('train/'):]].contiguous(), 'written ' + c[1])


def check_stacks_of(device, H=7, W=9):
  """stacks of 1, 6 and 7 flows: only the first 6 are used"""
  for n_flows in (1, 6, 7):
    check_panels(device, H, W, n_flows)


def check_refusals(device):
  """each is refused before a launch: wrong shapes or dtypes, more than 4 images or 12 flows per call, an unknown map name, unbuilt options"""
  import pytest
  from dynibar_amd import _lib, view_log
  x = torch.zeros((5, 6), dtype=torch.float32, device=device)
  f = torch.zeros((5, 6, 2), dtype=torch.float32, device=device)
  with pytest.raises(ValueError, match="'jet' and 'gray'"):
    view_log.colorize(x, 'viridis')
  for kw in (dict(mask=x > 0), dict(range=(0.0, 1.0)), dict(append_cbar=True)):
    with pytest.raises(NotImplementedError):
      view_log.colorize(x, 'jet', **kw)
  for bad in (x.double(), x[None], x[..., None].expand(5, 6, 2), torch.zeros((0, 6), dtype=torch.float32, device=device)):
    with pytest.raises(ValueError):
      view_log.colorize(bad)
  for bad in (f.double(), f[..., :1], x, f[None]):
    with pytest.raises(ValueError):
      view_log.flow_to_image(bad)
  with pytest.raises(ValueError, match='1..4'):
    view_log.ranges([x] * 5)
  with pytest.raises(ValueError, match='1..4'):
    view_log.ranges([])
  with pytest.raises(ValueError, match='1..12'):
    view_log.flow_max([f] * 13)
  with pytest.raises(ValueError, match='one size'):
    view_log.ranges([x, torch.zeros((6, 5), dtype=torch.float32, device=device)])
  # the library's own checks, before any launch
  import ctypes
  lib = _lib.lib()
  one = (ctypes.c_void_p * 1)(x.data_ptr())
  p = ctypes.cast(one, ctypes.c_void_p)
  flag = ctypes.cast((ctypes.c_int32 * 1)(0), ctypes.c_void_p)
  rank = (ctypes.c_int32 * 4)(0, 1, 28, 29)
  wt = (ctypes.c_double * 2)(0.29, 0.71)
  out = torch.zeros((4, 2), dtype=torch.float64, device=device)
  po = ctypes.c_void_p(out.data_ptr())
  rk, pw = ctypes.cast(rank, ctypes.c_void_p), ctypes.cast(wt, ctypes.c_void_p)
  assert lib.dyn_viewlog_ranges(5, 5, 6, p, flag, None, rk, pw, po, None) == -1 and b'5 images' in lib.dyn_last_error()
  assert lib.dyn_viewlog_ranges(1, 0, 6, p, flag, None, rk, pw, po, None) == -1 and b'unsupported' in lib.dyn_last_error()
  assert lib.dyn_viewlog_ranges(1, 5, 6, None, flag, None, rk, pw, po, None) == -1 and b'required' in lib.dyn_last_error()
  rank[3] = 30
  assert lib.dyn_viewlog_ranges(1, 5, 6, p, flag, None, rk, pw, po, None) == -1 and b'rank 3' in lib.dyn_last_error()
  rank[3] = 29
  wt[0] = 1.5
  assert lib.dyn_viewlog_ranges(1, 5, 6, p, flag, None, rk, pw, po, None) == -1 and b'weight 0' in lib.dyn_last_error()
  assert lib.dyn_viewlog_flow_max(13, 5, 6, p, po, None) == -1 and b'13 flows' in lib.dyn_last_error()
  assert lib.dyn_viewlog_flow_max(1, 5, 6, None, po, None) == -1 and b'required' in lib.dyn_last_error()
  assert lib.dyn_viewlog_panels(None, None) == -1 and b'null params' in lib.dyn_last_error()
  for kw, msg in ((dict(n_map=5), b'5 colour-mapped'), (dict(n_flow=13), b'13 flow'), (dict(n_rgb=9), b'9 rgb'), (dict(), b'no panel'),
                  (dict(n_rgb=1), b'rgb_src')):
    q = _lib.params('DynViewLogPanelsParams', H=5, W=6, **kw)
    assert lib.dyn_viewlog_panels(ctypes.byref(q), None) == -1 and msg in lib.dyn_last_error(), (kw, lib.dyn_last_error())
  assert bool((out == 0).all()), 'a refused call wrote something'


def _dct_basis(K, T):
  b = np.zeros((T, K), np.float32)
  for t in range(T):
    for k in range(1, K + 1):
      b[t, k - 1] = np.sqrt(2.0 / T) * np.cos(np.pi / (2.0 * T) * (2 * t + 1) * k)
  return torch.from_numpy(b)


class _MapsOf(object):
  """stands where a feature encoder stands (the real one needs 16 x 16 images at least): N images -> the first N of its seeded maps, cyclically"""

  def __init__(self, maps, state):
    self.maps, self.state, self.calls = maps, state, []

  def __call__(self, x):
    self.calls.append((tuple(x.shape), self.state['mode']))
    return self.maps[torch.arange(x.shape[0], device=self.maps.device) % self.maps.shape[0]].contiguous(), None


def check_log_view(device, H=12, W=16, num_vv=2, idx=4):
  """log_view on the 12 x 16 anchor scene of parity.check_render_image_mono_train (its weights' shapes and its feature maps), the frame served
  from a DeviceScene as in scene_cases: the panels equal the restatement applied to the same call's ret, the encoders and the render ran in
  eval mode, the model is back in training mode afterwards"""
  import types
  import cases
  import objective_cases as oc
  import scene_cases as sc
  from dynibar_amd import projection, synthetic as syn, view_log
  scn, _, _, _ = cases.anchor_case({k: cases.t(v) for k, v in syn.make_scene(seed=4, H=H, W=W, V=7, n_static=8, smooth=True).items()}, 2, 1)
  scene = sc.device_scene(device, H, W, 1)
  plan, _ = sc.planned(H, W, 1, num_vv, idx)
  state = {'mode': 'train', 'switches': []}

  def switch(mode):
    state['mode'] = mode
    state['switches'].append(mode)

  model = types.SimpleNamespace(net_coarse_st=syn.make_weights('static', 0), net_coarse_dy=syn.make_weights('dynamic', 0),
                                motion_mlp=syn.make_weights('motion', 0, num_basis=cases.NUM_BASIS),
                                trajectory_basis=_dct_basis(cases.NUM_BASIS, cases.NUM_FRAMES).to(device),
                                feature_net=_MapsOf(torch.cat([scn['featmaps'], scn['featmaps_anchor']]).to(device), state),
                                feature_net_st=_MapsOf(scn['static_featmaps'].to(device), state),
                                switch_to_eval=lambda: switch('eval'), switch_to_train=lambda: switch('train'))
  args = oc.args_of(anti_alias_pooling=0, mask_rgb=1, occ_weights_mode=0, num_vv=num_vv, chunk_size=80, N_samples=16, inv_uniform=True, N_importance=0,
                    white_bkgd=False)
  td = plan['train_data']
  ref_idx, anchor_idx = int(td['id'].item()), int(td['anchor_id'].item())
  ref_off = [int(i - ref_idx) for i in td['nearest_pose_ids'].squeeze().tolist()]
  anchor_off = [int(i - anchor_idx) for i in td['anchor_nearest_pose_ids'].squeeze().tolist()]
  sampler = scene.sampler(plan)
  seen = {}
  real_panels = view_log.panels

  def recording_panels(ret, gt_img, gt_disp, gt_flows):
    seen.update(ret=ret, gt=(gt_img, gt_disp, gt_flows))
    return real_panels(ret, gt_img, gt_disp, gt_flows)

  view_log.panels = recording_panels
  try:
    got = view_log.log_view(sampler, model, projection.Projector(device), args, len(ref_off) + num_vv, (ref_idx, anchor_idx),
                            (td['ref_time'].to(device), td['anchor_time'].to(device)), (ref_off, anchor_off))
  finally:
    view_log.panels = real_panels
  assert state['switches'] == ['eval', 'train'] and state['mode'] == 'train'
  assert [m for _, m in model.feature_net.calls + model.feature_net_st.calls] == ['eval', 'eval']
  assert not hasattr(args, 'frame_outputs'), 'log_view changed the caller\'s args'
  ret = seen['ret']
  need = {'outputs_coarse_ref': ('rgb', 'rgb_static', 'rgb_dy', 'depth', 'exp_sf', 'render_flows'), 'outputs_coarse_st': ('rgb',),
          'outputs_coarse_anchor': ('rgb', 'occ_weight_map')}
  host = OrderedDict((g, OrderedDict((k, ret[g][k].cpu()) for k in ks)) for g, ks in need.items())
  gt_img, gt_disp, gt_flows = (t.cpu() for t in seen['gt'])
  assert tuple(gt_img.shape) == (H, W, 3) and tuple(gt_disp.shape) == (H, W, 1) and gt_flows.shape[0] == 6
  for g in host.values():
    assert all(bool(torch.isfinite(v).all()) for v in g.values())
  assert float(host['outputs_coarse_ref']['rgb'].std()) > 1e-3, 'the rendered frame must not be flat'
  check_panel_values(got, panels_restated(host, gt_img, gt_disp, gt_flows), 6, H, W)
