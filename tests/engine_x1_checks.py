"""Checks of the one-product half-float engine build (libdynibar_hip_x1.so, dynibar_amd.engine 'half'; csrc/dyn_mlp.h DYN_SPLIT_TERMS == 1), shared by
tests/test_gpu_engine_x1.py (child processes on the device: a process binds one library) and tests/emu/test_emu_engine_x1.py (the wave-level emulator).

No tolerance here is chosen for the kernels.  The engine multiplies half-rounded operands exactly and accumulates in fp32, so
  (a) the engine self-test is compared with float64 arithmetic ON HALF-ROUNDED OPERANDS at the fp32-class limit of parity.check_mlp_selftest (3e-6:
      accumulation order) plus the derived effect of a hidden activation that sits on a rounding midpoint of the half grid and may round the other way;
  (b) the networks are compared with the float64 oracle (the exact value) next to the fp32 oracle whose Linear layers and attention products round both
      operands to half (`half_rounded_oracle`): per output the kernels' error is held to twice that oracle's own error plus 2e-6 of the output's scale --
      the idiom of parity._accuracy_table.  What the kernels keep in fp32 (pooling weights, mean / variance, row_dot layers, softmax, ELU, the long-ray
      attention) only makes them closer;
  (c) render_rays_mv is compared with the real reference's golden outputs in the same way.

  python tests/engine_x1_checks.py CHECK [CASE]     # what the device tests start as a child; prints the tables, then `x1-check ok`
"""
import contextlib
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import cases
import parity
from dynibar_amd import _lib, ops
from oracle import ibr_oracle as O
from parity import cpu, to_dev

HALF_MAX = 65504.0


def rn(x):
  """round to the nearest IEEE half (ties to even), saturating at +-65504; the result keeps x's dtype"""
  return x.clamp(-HALF_MAX, HALF_MAX).to(torch.float16).to(x.dtype)


def ulp_half(v):
  """spacing of the half grid at |v| (2^-24 in the subnormal range)"""
  a = v.abs().double().clamp_min(2.0 ** -14)
  return torch.exp2(torch.floor(torch.log2(a)) - 10.0)


def near_midpoint(v, window):
  """|v| lies within `window` of a point halfway between two neighbouring halves"""
  u = ulp_half(v)
  frac = torch.remainder(v.abs().double() / u, 1.0)
  return ((frac - 0.5).abs() * u) <= window


def require_x1():
  terms, kind = _lib.lib().dyn_mlp_split_terms(), _lib.lib().dyn_mlp_split_kind()
  assert terms == 1 and kind == 2, f'this check is for the one-product half-float build; the bound library has split terms {terms}, kind {kind}'


# ---- (a) engine self-test -------------------------------------------------------------------------------------------------------------------
def _selftest(device, W, b, x):
  xd = x.to(device)
  y = torch.full(tuple(x.shape), float('nan'), device=device)
  buf = torch.zeros(2 * 3 * 4096, device=device)
  _lib.call('dyn_mlp_selftest', ctypes.c_void_p(W.data_ptr()), ctypes.c_void_p(b.data_ptr()), _lib.ptr(xd), _lib.ptr(y), x.shape[0], _lib.ptr(buf), _lib.stream_of(xd))
  return cpu(y)


def _rounded_reference(W, b, x, round_input=True):
  """float64 on half-rounded operands: h1 = elu(linear(rn(x), rn(W), b)), ref = elu(linear(rn(h1), rn(W), b)); and the per-element allowance for a
  hidden activation within 4e-6 of a rounding midpoint rounding the other way: sum_k |rn(W)[n, k]| ulp_half(h1[r, k])"""
  Wr, bd = rn(W).double(), b.double()
  h1 = F.elu(F.linear(rn(x).double() if round_input else x.double(), Wr, bd))
  ref = F.elu(F.linear(rn(h1), Wr, bd))
  flip = F.linear(ulp_half(h1) * near_midpoint(h1, 4e-6).double(), Wr.abs())
  return h1, ref, flip


def check_selftest(device, rows=1000):
  """the inputs of parity.check_mlp_selftest; limit 3e-6 (accumulation order) + the midpoint term, no element excluded"""
  require_x1()
  g = torch.Generator().manual_seed(0)
  W = (torch.rand(64, 64, generator=g) - 0.5) * 0.4
  b = torch.rand(64, generator=g) - 0.5
  x = torch.randn(rows, 64, generator=g)
  y = _selftest(device, W, b, x)
  _, ref, flip = _rounded_reference(W, b, x)
  err = (y.double() - ref).abs()
  lim = 3e-6 + flip
  plain = F.elu(F.linear(F.elu(F.linear(x, W, b)), W, b)).double()
  quiet = flip == 0
  print(f'  x1 engine self-test, {rows} rows: max err against float64 on half-rounded operands {float(err.max()):.3e}; elements without a near-midpoint hidden value '
        f'{int(quiet.sum())}/{quiet.numel()}, their max err {float(err[quiet].max()):.3e}; over the limit {int((err > lim).sum())}; '
        f'distance from the plain fp32 reference {float((y.double() - plain).abs().max()):.3e}', flush=True)
  parity.record_margin(f'x1 engine self-test ({rows} rows) against float64 on half-rounded operands', err, lim)
  assert int((err > lim).sum()) == 0, f'x1 engine self-test: {int((err > lim).sum())}/{err.numel()} elements over 3e-6 + midpoint term, worst excess {float((err - lim).max()):.3e}'
  return float(err.max())


def check_selftest_ranges(device, rows=512):
  """the `tiny` and `huge` ranges of parity.check_mlp_selftest_ranges (same seed, same draws).  Outputs must be finite.  tiny: activations of 1e-6 .. 6e-5 enter
  on the SUBNORMAL half grid (2^-24 absolute): against float64 with the tiny input NOT rounded (weights and the O(1) hidden operand are half-rounded as in
  the self-test: no one-product engine can do without that), the limit is 2^-24 sum_k |w| per element plus the midpoint term of the self-test.  huge
  (7e4 .. 1.2e5, beyond the largest half: the operand saturates at 65504) is measured and recorded, finite outputs asserted."""
  require_x1()
  g = torch.Generator().manual_seed(3)
  W0 = (torch.rand(64, 64, generator=g) - 0.5) * 0.4
  b = torch.rand(64, generator=g) - 0.5
  out = {}
  for tag, lo, hi, wscale in (('tiny', 1e-6, 6e-5, 1.0), ('huge', 7e4, 1.2e5, 0.15)):
    W = (W0 * wscale).contiguous()
    mag = lo + (hi - lo) * torch.rand(rows, 64, generator=g)
    x = mag * torch.where(torch.rand(rows, 64, generator=g) < 0.5, -1.0, 1.0)
    y = _selftest(device, W, b, x)
    assert bool(torch.isfinite(y).all()), f'{tag} activations: non-finite output'
    h1, ref, flip = _rounded_reference(W, b, x, round_input=False)
    err = (y.double() - ref).abs()
    exact = F.elu(F.linear(F.elu(F.linear(x.double(), W.double(), b.double())), W.double(), b.double()))
    scale = F.linear(h1.abs(), W.double().abs(), b.double().abs())
    out[tag] = float(err.max())
    print(f'  x1 engine, activations {lo:g}..{hi:g} (hidden up to {float(h1.abs().max()):.3g}): max err against float64 on half-rounded weights and hidden operand '
          f'{float(err.max()):.3e}; against plain float64 {float((y.double() - exact).abs().max()):.3e} = {float(((y.double() - exact).abs() / scale).max()):.2e} of sum|w||h|', flush=True)
    if tag == 'tiny':
      lim = 2.0 ** -24 * rn(W).double().abs().sum(dim=1)[None, :] + flip
      parity.record_margin('x1 engine, tiny activations: subnormal half grid', err, lim.expand_as(err))
      assert bool((err <= lim).all()), f'tiny activations: {int((err > lim).sum())} elements over 2^-24 sum|w| + midpoint term, worst excess {float((err - lim).max()):.3e}'
  return out


# ---- (b) the half-rounded oracle ------------------------------------------------------------------------------------------------------------------
class _TorchWithRoundedMatmul:
  """stands in for the oracle module's `torch` while one of its networks runs: matmul (the two attention products) rounds both operands to half"""

  def __getattr__(self, name):
    return getattr(torch, name)

  @staticmethod
  def matmul(a, b):
    return torch.matmul(rn(a), rn(b))


@contextlib.contextmanager
def half_rounded_oracle():
  """Inside: O.static_net, O.dynamic_net and O.motion_mlp multiply like the one-product engine -- every Linear rounds its input and its weight to the nearest
  half before F.linear (fp32 accumulation, fp32 bias), the attention products round both operands.  Only while one of those three runs: projection, sampling
  and compositing are untouched.  The oracle's files are not edited; everything is restored on exit."""
  saved = {n: getattr(O, n) for n in ('static_net', 'dynamic_net', 'motion_mlp')}

  def rounded(fn):
    def run(*a, **kw):
      lin, tm = O._lin, O.torch
      O._lin = lambda sd, name, x: F.linear(rn(x), rn(sd[name + '.weight']), sd.get(name + '.bias'))
      O.torch = _TorchWithRoundedMatmul()
      try:
        return fn(*a, **kw)
      finally:
        O._lin, O.torch = lin, tm
    return run

  for n, fn in saved.items():
    setattr(O, n, rounded(fn))
  try:
    yield
  finally:
    for n, fn in saved.items():
      setattr(O, n, fn)


def _f64(x):
  if isinstance(x, dict):
    return {k: _f64(v) for k, v in x.items()}
  if isinstance(x, (list, tuple)):
    return type(x)(_f64(v) for v in x)
  return x.double() if isinstance(x, torch.Tensor) and x.is_floating_point() else x


def _in_double(fn, *args, **kw):
  prev = torch.get_default_dtype()
  torch.set_default_dtype(torch.float64)  # the oracle's linspace / ones / tensor constructors follow the default dtype
  try:
    return fn(*_f64(args), **_f64(kw))
  finally:
    torch.set_default_dtype(prev)


def accuracy_table(tag, ours, ref, exact, sigma_in=()):
  """The figures of parity._accuracy_table printed in full BEFORE anything is asserted (per output the kernels' and the half-rounded oracle's absolute
  error against `exact`: largest, 99th, 90th percentile), then parity._accuracy_table itself: the rule -- twice the reference's figures plus 2e-6 of the
  output's scale; largest, p99 and p90 where there are >= 2000 elements, p90 below -- lives there alone."""
  for k in ours:
    t64 = exact[k].double()
    live = torch.ones_like(t64, dtype=torch.bool)
    if k in sigma_in:
      live = live & (t64[..., 3:4] > -1e8)  # points without a valid view: sigma is the constant -1e9 on every side (asserted by the caller)
    e_ref, e_our = (ref[k].double() - t64).abs()[live], (ours[k].double() - t64).abs()[live]
    q = lambda e, p: float(torch.quantile(e.flatten()[:: max(1, e.numel() // 200000)], p))
    print(f'  x1 accuracy [{tag}] {k} (n {e_ref.numel()}, scale {float(t64[live].abs().max()):.3g}): kernels max {float(e_our.max()):.2e} p99 {q(e_our, 0.99):.2e} '
          f'p90 {q(e_our, 0.9):.2e} | half-rounded oracle max {float(e_ref.max()):.2e} p99 {q(e_ref, 0.99):.2e} p90 {q(e_ref, 0.9):.2e}', flush=True)
  return parity._accuracy_table(tag, list(ours), ours, ref, {k: v.double() for k, v in exact.items()}, Ellipsis, sigma_in=sigma_in)


def _dead_sigma_exact(raw, raw_ref, what):
  dead = raw_ref[..., 3] < -1e8
  assert bool((raw[..., 3][dead] == raw_ref[..., 3][dead]).all()) and bool((raw_ref[..., 3][dead] == -1e9).all()), f'{what}: sigma of points without a valid view must be -1e9 exactly'
  return int(dead.sum())


def check_static_net(device, name='small', S=64, R=None, aa=True, mask_rgb=False, weights='init', dark=0.0):
  """DynibarStatic on the oracle's own stage inputs (parity.check_static_net's inputs, its `dark` rows included)"""
  require_x1()
  scene, o, d, sd, _, st = parity.static_inputs(name, S, R, weights)
  assert R is None or o.shape[0] == R, f'scene {name} has {o.shape[0]} rays, the case asks for {R}'
  if dark > 0.0:
    g = torch.Generator().manual_seed(77)
    rf = st['rgb_feat'].clone()
    row_dark = torch.rand(rf.shape[:3], generator=g) < dark
    row_dark |= (torch.rand(rf.shape[:2], generator=g) < 0.1 * dark + 0.02)[..., None]
    rf[..., :3] = torch.where(row_dark[..., None], torch.zeros(()), rf[..., :3])
    st = dict(st, rgb_feat=rf)
  net_args = (sd, st['pts'], st['ref_rays_coords'], st['src_rays_coords'], st['rgb_feat'], F.normalize(d, dim=-1), st['ray_diff'], st['mask'])
  with half_rounded_oracle():
    raw_h = O.static_net(*net_args, aa, mask_rgb)
  raw_64 = _in_double(O.static_net, *net_args, aa, mask_rgb)
  sdev = to_dev(scene, device)
  views = ops.SourceViews(sdev['camera'], sdev['static_src_rgbs'], sdev['static_src_cameras'], sdev['static_featmaps'])
  net = ops.StaticNet(parity._weights(weights)['net_coarse_st'], device, aa, mask_rgb)
  raw = cpu(net(views, o.to(device), d.to(device), st['pts'].to(device), st['rgb_feat'].to(device), st['ray_diff'].to(device), st['mask'].to(device)))
  tag = f'static net {name}, {weights} weights, R={o.shape[0]} S={S}' + (f', mask_rgb dark {dark}' if dark else '')
  n_dead = _dead_sigma_exact(raw, raw_h, tag)
  return dict(accuracy_table(tag, dict(raw=raw), dict(raw=raw_h), dict(raw=raw_64), sigma_in=('raw',)), dead_points=n_dead)


def check_dynamic_net(device, name='small', S=64, R=None, shift=0.0, weights='init'):
  require_x1()
  di = parity.dynamic_inputs(name, S, R, weights)
  assert R is None or di['pts'].shape[0] == R, f'scene {name} has {di["pts"].shape[0]} rays, the case asks for {R}'
  Vd = di['rgb_feat'].shape[2]
  tdiff = torch.zeros(di['pts'].shape[0], S, Vd, 1)
  net_args = (di['W']['net_coarse_dy'], di['pts'], di['rgb_feat'], F.normalize(di['d'], dim=-1), di['ray_diff'], tdiff, di['mask'], di['t_emb'])
  with half_rounded_oracle():
    raw_h = O.dynamic_net(*net_args, shift=shift)
  raw_64 = _in_double(O.dynamic_net, *net_args, shift=shift)
  net = ops.DynamicNet(parity._weights(weights)['net_coarse_dy'], device, shift=shift)
  raw = cpu(net(di['d'].to(device), di['pts'].to(device), di['rgb_feat'].to(device), di['mask'].to(device), di['temb'].to(device)))
  tag = f'dynamic net {name}, {weights} weights, R={di["pts"].shape[0]} S={S}, shift {shift}'
  n_dead = _dead_sigma_exact(raw, raw_h, tag)
  return dict(accuracy_table(tag, dict(raw_dy=raw), dict(raw_dy=raw_h), dict(raw_dy=raw_64), sigma_in=('raw_dy',)), dead_points=n_dead)


def check_motion(device, name='small', S=64, R=None, weights='init'):
  require_x1()
  di = parity.dynamic_inputs(name, S, R, weights)
  assert R is None or di['pts'].shape[0] == R, f'scene {name} has {di["pts"].shape[0]} rays, the case asks for {R}'
  xin = torch.cat([di['pts'], di['t_emb']], -1).float()
  with half_rounded_oracle():
    c_h = O.motion_mlp(di['W']['motion_mlp'], xin)
  c_64 = _in_double(O.motion_mlp, di['W']['motion_mlp'], xin)
  keep = S - di['n_last']
  mm = ops.MotionMLP(parity._weights(weights)['motion_mlp'], device, cases.NUM_BASIS)
  coeff = cpu(mm(di['pts'].to(device), di['temb'].to(device), di['n_last']))
  assert bool((coeff[:, keep:] == 0).all()), 'the last samples of every ray carry no motion'
  return accuracy_table(f'motion MLP {name}, {weights} weights, R={xin.shape[0]} S={S}', dict(coeff=coeff[:, :keep]), dict(coeff=c_h[:, :keep]), dict(coeff=c_64[:, :keep]))


def check_cross_axis(device, name):
  """the two shapes of tests/golden/cross_axis.npz (3 static views; 3 rays x 3 samples): DynibarStatic, both argument sets of the golden"""
  S = cases.CROSS_AXIS_SAMPLES[name]
  return [check_static_net(device, name, S=S, aa=bool(aa), mask_rgb=bool(mr)) for aa, mr in ((1, 0), (0, 1))]


# the device cases: the smallest on which each kernel form can go wrong (name -> callable(device))
NETWORK_CASES = {
    'static_small_s32': lambda dev: check_static_net(dev, 'small', S=32),                      # lane-segment views
    'static_small_s64': lambda dev: check_static_net(dev, 'small', S=64),
    'static_harsh_dark': lambda dev: check_static_net(dev, 'harsh', S=32, R=4, mask_rgb=True, dark=0.4),  # 11 views: ragged dense rows, mask_rgb removes rows and points
    'many_views': lambda dev: (check_static_net(dev, 'many', S=16, R=3), check_dynamic_net(dev, 'many', S=16, R=3)),  # 20 static / 13 dynamic views
    'dynamic_small_shift': lambda dev: check_dynamic_net(dev, 'small', S=64, shift=5.0),
    'motion_small': lambda dev: check_motion(dev, 'small', S=64),
    # 12 rays of a scene that has them (48): several workgroups of every chain
    'several_workgroups': lambda dev: (check_static_net(dev, 'harsh_many', S=32, R=12), check_dynamic_net(dev, 'harsh_many', S=32, R=12, shift=5.0)),
    'long_rays_s160': lambda dev: (check_static_net(dev, 'small', S=160, R=3), check_dynamic_net(dev, 'small', S=160, R=3, shift=5.0)),  # the two-launch point chain
    'cross_views': lambda dev: check_cross_axis(dev, 'cross_views'),
    'cross_rays_samples': lambda dev: check_cross_axis(dev, 'cross_rays_samples'),
    'trained_small': lambda dev: check_static_net(dev, 'small', S=48, R=5, weights='trained'),  # the pooling-weight cancellation: where narrow operands hurt most
}
# their twins under the emulator (one or two rays, 16 or 32 samples)
EMU_CASES = {
    'static_small': lambda dev: check_static_net(dev, 'small', S=32, R=1),
    'static_harsh_dark': lambda dev: check_static_net(dev, 'harsh', S=32, R=2, mask_rgb=True, dark=0.4),
    'many_views': lambda dev: (check_static_net(dev, 'many', S=16, R=1), check_dynamic_net(dev, 'many', S=16, R=1)),
    'dynamic_small_shift': lambda dev: check_dynamic_net(dev, 'small', S=32, R=1, shift=5.0),
    'motion_small': lambda dev: check_motion(dev, 'small', S=32, R=1),
    'cross_views': lambda dev: check_cross_axis(dev, 'cross_views'),
    'cross_rays_samples': lambda dev: check_cross_axis(dev, 'cross_rays_samples'),
    'trained_small': lambda dev: check_static_net(dev, 'small', S=16, R=2, weights='trained'),
}


# ---- (c) path level ---------------------------------------------------------------------------------------------------------------------------
def _render_rays_mv(device, name='small', S=64):
  import types
  from dynibar_amd import projection, render_ray
  scene, o, d, uv, _ = cases.scene_case(name)
  fidx, temb, toff = cases.time_args(scene['src_rgbs'].shape[1])
  model = parity.make_model(device)
  args = types.SimpleNamespace(anti_alias_pooling=True, mask_rgb=False, occ_weights_mode=0)
  batch = parity.make_ray_batch(scene, o, d, uv, device)
  cfeat = (scene['featmaps'].to(device), None, scene['static_featmaps'].to(device))
  ffeat = (scene['featmaps_fine'].to(device), None, scene['static_featmaps_fine'].to(device))
  return render_ray.render_rays_mv((fidx, None), (temb.to(device), None), (toff, None), batch, model, projection.Projector(device), cfeat, ffeat, S, args,
                                   inv_uniform=True, N_importance=S, det=True, is_train=False)


def check_render_rays_mv(device, golden, name='small', S=64):
  """render_rays_mv (coarse 64 + fine 64, both branches) on the golden scene of the real reference: rgb / depth / weights of every output group held to
  twice the half-rounded oracle's distance from the same golden; two identical calls give identical bits.  Prints the plain maximum |rgb error|."""
  require_x1()
  ret = _render_rays_mv(device, name, S)
  again = _render_rays_mv(device, name, S)
  scene, o, d, uv, _ = cases.scene_case(name)
  fidx, temb, toff = cases.time_args(scene['src_rgbs'].shape[1])
  with half_rounded_oracle():
    ref = O.render_rays_mv(parity.oracle_models(), dict(scene), o, d, uv, fidx, temb, toff, S, S)
  worst_rgb, n_same = 0.0, 0
  for grp in ('outputs_coarse_ref', 'outputs_fine_ref', 'outputs_fine_ref_dy'):
    for k, v in ret[grp].items():
      if isinstance(v, torch.Tensor):
        parity.assert_bitexact(cpu(again[grp][k]), cpu(v), f'x1 render_rays_mv, second identical call: {grp}/{k}')
        n_same += 1
    keys = [k for k in ('rgb', 'depth', 'weights') if ret[grp].get(k) is not None and f'mv/{grp}/{k}' in golden]
    gold = {k: torch.from_numpy(golden[f'mv/{grp}/{k}']) for k in keys}
    accuracy_table(f'render_rays_mv {name} {grp} against the real reference', {k: cpu(ret[grp][k]) for k in keys}, {k: ref[grp][k] for k in keys}, gold)
    if 'rgb' in keys:
      worst_rgb = max(worst_rgb, float((cpu(ret[grp]['rgb']) - gold['rgb']).abs().max()))
  print(f'  x1 render_rays_mv {name}: max |rgb error| against the real reference {worst_rgb:.3e} (8-bit step 3.9e-3); {n_same} tensors bit-identical in a second call', flush=True)
  return worst_rgb


def check_chunk_streams(device, H=64, W=96, chunk_size=1024):
  """a 64 x 96 frame of render_single_image_nvi with its chunks on one and on two streams: identical bits in every entry"""
  import types
  from dynibar_amd import projection, render_image, sample_ray, synthetic as syn
  require_x1()
  cfg = dict(seed=4, H=H, W=W, V=7, n_static=8, smooth=True)
  sc, fine = syn.make_scene(**cfg), syn.make_scene(**dict(cfg, tag=1))
  scene = {k: cases.t(v) for k, v in sc.items()}
  data = dict(camera=scene['camera'], rgb_path='x', depth_range=scene['depth_range'], src_rgbs=scene['src_rgbs'], src_cameras=scene['src_cameras'],
              static_src_rgbs=scene['static_src_rgbs'], static_src_cameras=scene['static_src_cameras'])
  cfeat = (scene['featmaps'].to(device), None, scene['static_featmaps'].to(device))
  ffeat = (cases.t(fine['featmaps']).to(device), None, cases.t(fine['static_featmaps']).to(device))
  smp = sample_ray.RaySamplerSingleImage(data, device)
  rb = smp.get_all()
  model = parity.make_model(device)
  args = types.SimpleNamespace(anti_alias_pooling=True, mask_rgb=False, occ_weights_mode=0, frame_outputs='all')
  fidx, temb, toff = cases.time_args(7)
  outs, prev = [], render_image.CHUNK_STREAMS
  try:
    for n in (1, 2):
      render_image.CHUNK_STREAMS = n
      ret = render_image.render_single_image_nvi((fidx, None), (temb.to(device), None), (toff, None), smp, rb, model, projection.Projector(device), chunk_size, 64,
                                                 args, inv_uniform=True, N_importance=64, det=True, coarse_featmaps=cfeat, fine_featmaps=ffeat, is_train=False)
      outs.append({(g, k): v.clone() for g in ('outputs_coarse_ref', 'outputs_fine_ref') for k, v in ret[g].items() if isinstance(v, torch.Tensor)})
  finally:
    render_image.CHUNK_STREAMS = prev
  assert tuple(outs[0][('outputs_fine_ref', 'rgb')].shape[:2]) == (H, W)
  for key, v in outs[0].items():
    parity.assert_bitexact(outs[1][key], v, f'x1 frame, two chunk streams against one: {key}')
  print(f'  x1 frame {H} x {W}, chunks of {chunk_size} rays: {len(outs[0])} tensors bit-identical on one and on two chunk streams', flush=True)
  return len(outs[0])


# ---- (d) interface ------------------------------------------------------------------------------------------------------------------------------
def check_interface_env():
  """run with DYNIBAR_ENGINE=half and no DYNIBAR_HIP_LIB: the environment selects the library; a second choice after the library is bound is refused"""
  from dynibar_amd import engine
  assert not os.environ.get('DYNIBAR_HIP_LIB') and os.environ.get('DYNIBAR_ENGINE') == 'half'
  cur = engine.current()
  assert cur['terms'] == 1 and cur['kind'] == 2 and cur['name'] == 'half' and os.path.basename(cur['path']) == 'libdynibar_hip_x1.so', cur
  try:
    engine.select('split')
  except RuntimeError as e:
    assert 'libdynibar_hip_x1.so' in str(e), e
  else:
    raise AssertionError('engine.select after the library is bound must raise')
  print('  DYNIBAR_ENGINE=half ->', json.dumps(cur))


def check_interface_select(device):
  """engine.select('half') before the first kernel call binds the x1 library; engine.select after a kernel call raises, naming the loaded library"""
  from dynibar_amd import engine
  assert not os.environ.get('DYNIBAR_HIP_LIB') and not os.environ.get('DYNIBAR_ENGINE')
  try:
    engine.select('fast')
  except ValueError:
    pass
  else:
    raise AssertionError('an unknown engine name must be a ValueError')
  engine.select('half')
  z = ops.sample_along_ray(torch.zeros(4, 3, device=device), torch.ones(4, 3, device=device), torch.tensor([[1.0, 2.0]], device=device), 8, True)[1]
  assert tuple(z.shape) == (4, 8)
  cur = engine.current()
  assert cur['terms'] == 1 and cur['name'] == 'half', cur
  for name in ('half', 'split'):
    try:
      engine.select(name)
    except RuntimeError as e:
      assert 'libdynibar_hip_x1.so' in str(e), e
    else:
      raise AssertionError('engine.select after a kernel call must raise')
  print('  engine.select("half") ->', json.dumps(cur))


def check_interface_lib_wins():
  """run with DYNIBAR_ENGINE=half AND DYNIBAR_HIP_LIB = the default library: the explicit path wins"""
  from dynibar_amd import engine
  try:
    engine.select('half')  # (nothing is bound yet: the refusal is the explicit path's)
  except RuntimeError as e:
    assert 'DYNIBAR_HIP_LIB' in str(e), e
  else:
    raise AssertionError('engine.select must not override an explicit DYNIBAR_HIP_LIB')
  engine.select('split')  # the flavour the explicit path already names is no conflict
  cur = engine.current()
  assert cur['path'] == os.environ['DYNIBAR_HIP_LIB'] and cur['terms'] == 3 and cur['name'] == 'split', cur
  print('  DYNIBAR_HIP_LIB over DYNIBAR_ENGINE ->', json.dumps(cur))


def main(argv):
  dev = 'cuda:0'
  what = argv[0]
  golden_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
  if what == 'selftest':
    check_selftest(dev, 1000)
    check_selftest_ranges(dev)
  elif what == 'network':
    NETWORK_CASES[argv[1]](dev)
  elif what == 'path':
    check_render_rays_mv(dev, dict(np.load(os.path.join(golden_dir, 'stages_small.npz'))), 'small')
  elif what == 'streams':
    check_chunk_streams(dev)
  elif what == 'interface_env':
    check_interface_env()
  elif what == 'interface_select':
    check_interface_select(dev)
  elif what == 'interface_lib_wins':
    check_interface_lib_wins()
  else:
    raise SystemExit(f'unknown check {what}')
  if dev == 'cuda:0' and torch.cuda.is_initialized():
    torch.cuda.synchronize()
  print('x1-check ok')


if __name__ == '__main__':
  main(sys.argv[1:])
