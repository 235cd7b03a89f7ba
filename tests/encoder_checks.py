"""Checks of the feature encoder (csrc/dyn_encoder.hip) where its work split and its statistics matter, parameterised by device like
tests/parity.py: 'cuda:0' runs libdynibar_hip.so on an MI355X (-m gpu), 'cpu' the same sources under the wave-level emulator (tests/emu).

The reference of every check is the oracle's restatement of the executed part of ResNet.forward (oracle/ibr_oracle.py:resnet_encoder, pinned to the
real reference's outputs by the encoder goldens) evaluated in float64 on the CPU.

  conv_split                  how launch_conv / k_enc_conv divide the N * Hout output rows over the workgroups, restated
  check_encoder_regime        forward kernels on a shape chosen for the regime of that split it reaches; the regime is asserted first
  check_encoder_conditioning  low-contrast frames (|mean| / std of a channel in the hundreds): held to twice the fp32 oracle's own error
  check_im2col / check_col2im / check_instance_norm / check_helper_argument_errors    the training form's exported helpers on their own
"""
import ctypes
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import cases
import parity
from dynibar_amd import _lib, ops
from oracle import ibr_oracle as O

EMU_CUS = 7  # what tests/emu/hip/hip_runtime.h reports as multiProcessorCount


def cu_count(device):
  return torch.cuda.get_device_properties(0).multi_processor_count if str(device).startswith('cuda') else EMU_CUS


WAVES = 8  # ENC_THREADS / 64: wave w of a workgroup takes tiles w, w + 8, ... of its run (tile = 32 pixels of a row, row-major)


def conv_split(N, Hout, Wout, cu):
  """launch_conv + k_enc_conv restated: rows = N * Hout flattened (image, output row) pairs, grid = min(rows, max(cu, N)) workgroups, workgroup b owns
  rows [rows * b // grid, rows * (b + 1) // grid).  -> dict(rows, grid, runs, min_len, max_len, crossing = runs that touch two images,
  switching = wavefronts that write pixels of two images: they flush their statistics and change the coefficient table between two tiles)."""
  rows = N * Hout
  grid = min(rows, max(cu, N))
  runs = [(rows * b // grid, rows * (b + 1) // grid) for b in range(grid)]
  lens = [hi - lo for lo, hi in runs]
  crossing = sum(1 for lo, hi in runs if hi > lo and lo // Hout != (hi - 1) // Hout)
  assert all(hi > lo and (hi - 1) // Hout - lo // Hout <= 1 for lo, hi in runs), 'a run spans more than two images: the kernel tabulates two'
  tiles_x = (Wout + 31) // 32
  switching = 0
  for lo, hi in runs:
    if lo // Hout != (hi - 1) // Hout:
      for w in range(WAVES):
        imgs = {(lo + tile // tiles_x) // Hout for tile in range(w, (hi - lo) * tiles_x, WAVES)}
        switching += len(imgs) == 2
  return dict(rows=rows, grid=grid, runs=runs, min_len=min(lens), max_len=max(lens), crossing=crossing, switching=switching)


def encoder_sizes(H, W):
  """(H1, W1) of the half-resolution maps (conv 7x7 / 2, pad 3) and (H2, W2) of the quarter-resolution ones (3x3 / 2, pad 1)"""
  H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
  return (H1, W1), ((H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1)


def encoder_splits(N, H, W, cu):
  (H1, W1), (H2, W2) = encoder_sizes(H, W)
  return conv_split(N, H1, W1, cu), conv_split(N, H2, W2, cu)


# What each shape is FOR: predicates on (half-resolution split, quarter-resolution split, N).  They name a regime, not the figures of one CU count;
# the figures on 256 CUs are in the comments.  A device on which a predicate is false fails the test before anything is launched.
REGIMES = {
    # 2592 / 1296 rows: runs of 10-11 and 5-6 rows, 16 and 14 of them crossing an image
    # and wavefronts that switch image between two of their tiles at both resolutions
    'eval': lambda h, q, N: h['min_len'] >= 2 and q['min_len'] >= 2 and h['switching'] >= 1 and q['switching'] >= 1 and h['grid'] > N,
    # 1440 / 720 rows: runs of 5-6 and 2-3, 8 and 6 crossing
    'train': lambda h, q, N: h['min_len'] >= 2 and q['min_len'] >= 2 and h['switching'] >= 1 and q['crossing'] >= 1 and h['grid'] > N,
    # 518 rows in runs of 2-3 (3 crossing), 259 rows in runs of 1-2: one-row and two-row runs in the same launch
    'ragged': lambda h, q, N: h['min_len'] >= 2 and h['crossing'] >= 1 and q['min_len'] == 1 and q['max_len'] == 2,
    # 303 rows: runs of 1-2, none crossing; 153 rows: one row per workgroup
    'just_over': lambda h, q, N: h['min_len'] == 1 and h['max_len'] == 2 and h['crossing'] == 0 and q['max_len'] == 1,
    # more images than CUs: grid = N, every run exactly one image
    'many': lambda h, q, N: h['grid'] == N and q['grid'] == N and h['crossing'] == 0 and q['crossing'] == 0 and h['min_len'] == h['max_len'],
    # the smallest image the library takes: 8 and 4 rows, one each
    'min': lambda h, q, N: h['max_len'] == 1 and q['max_len'] == 1,
    # the emulator's twins (7 CUs)
    'small': lambda h, q, N: h['min_len'] >= 2 and h['crossing'] >= 1 and q['crossing'] >= 1,
    'odd': lambda h, q, N: h['crossing'] >= 2 and q['crossing'] >= 2,
    'nine': lambda h, q, N: h['grid'] == N and q['grid'] == N and h['crossing'] == 0,
    # 2 x 64 x 16: runs long enough at 1/2 resolution (9-10 one-tile rows) for a wavefront to take tiles of both images; on 'small' and 'odd'
    # runs do cross an image, but every wavefront gets one tile there, so no wavefront ever flushes sums of one image and goes on with the next
    'tall': lambda h, q, N: h['switching'] >= 1 and q['crossing'] >= 1,
}


def assert_regime(device, name, N, H, W):
  cu = cu_count(device)
  h, q = encoder_splits(N, H, W, cu)
  fig = lambda s: (f'{s["rows"]} rows over {s["grid"]} workgroups, runs of {s["min_len"]}-{s["max_len"]} rows, {s["crossing"]} crossing an image, '
                   f'{s["switching"]} wavefronts switching image')
  msg = f'encoder {name} {N} x {H} x {W} on {cu} CUs: 1/2 res {fig(h)}; 1/4 res {fig(q)}'
  assert REGIMES[name](h, q, N), 'the work-split regime this case is named for does not occur on this device -- ' + msg
  print('  ' + msg)
  return h, q


_REF64 = {}


def reference64(name, shape=None):
  """(imgs [N,H,W,3], weights, float64 coarse, float64 fine) of an encoder case, computed once per session"""
  key = (name, shape)
  if key not in _REF64:
    imgs, sd = cases.encoder_case(name, shape)
    p64 = {k: v.double() for k, v in O.tdict(sd).items()}
    with torch.no_grad():
      c64, f64 = O.resnet_encoder(p64, imgs.permute(0, 3, 1, 2).double())
    _REF64[key] = (imgs, sd, c64, f64)
  return _REF64[key]


def _where(err_over, shape, Hout, split):
  """flat index of the worst element of an NCHW map -> words: image, channel, output row, column, and where the row sits in its workgroup's run"""
  n, c, y, x = np.unravel_index(int(err_over), shape)
  row = n * Hout + y
  lo, hi = next(r for r in split['runs'] if r[0] <= row < r[1])
  place = 'the only row' if hi - lo == 1 else 'the first row' if row == lo else 'the last row' if row == hi - 1 else 'an interior row'
  return f'image {n}, channel {c}, output row {y}, column {x}: {place} of a run of {hi - lo} (rows {lo}..{hi - 1} of the flattened list)'


def assert_maps(got_c, got_f, c64, f64, what, split):
  """both maps, every element, 1e-4 + 1e-4 |ref| against float64 (check_encoder's limit); a failure names where in the work split it sits"""
  worst = 0.0
  for got, ref, key in ((got_c, c64, 'coarse'), (got_f, f64, 'fine')):
    assert tuple(got.shape) == tuple(ref.shape), f'{what} {key}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    assert ops._channels_last_view(got) is not None, f'{what} {key}: encoder outputs must be channels-last in memory'
    g = parity.cpu(got).double()
    assert bool(torch.isfinite(g).all()), f'{what} {key}: non-finite values'
    try:
      parity.assert_close(g, ref, 1e-4, 1e-4, f'{what} {key} vs float64')
    except AssertionError as e:
      over = (g - ref).abs() - (1e-4 + 1e-4 * ref.abs())
      raise AssertionError(f'{e}\n  worst: {_where(torch.argmax(over), ref.shape, ref.shape[2], split)}') from None
    worst = max(worst, float(((g - ref).abs() / (1e-4 + 1e-4 * ref.abs())).max()))
  return worst


def _holder(params):
  """an nn.Module around {name: tensor} with the reference's parameter names (what ResNet.from_module wraps)"""
  class Holder(torch.nn.Module):
    def __init__(self):
      super().__init__()
      self.p = torch.nn.ParameterDict({k.replace('.', '__'): torch.nn.Parameter(v.detach().clone()) for k, v in params.items()})

    def named_parameters(self, *a, **kw):
      return [(k.replace('__', '.'), v) for k, v in self.p.items()]

    def state_dict(self, *a, **kw):
      return {k.replace('__', '.'): v.detach() for k, v in self.p.items()}

  return Holder()


def check_encoder_regime(device, name, shape=None, other_entries=False, calls=2):
  """Forward-only kernels (ops.Encoder) on a case chosen for its work-split regime, asserted first; a second call on the same object (workspace
  reuse, statistics tables zeroed again) meets the same limit.  other_entries: also train_encoder.encoder_forward and the ResNet wrapper under
  no_grad.  Returns the largest fraction of the limit used."""
  from dynibar_amd import feature_network, train_encoder
  imgs, sd, c64, f64 = reference64(name, shape)
  N, H, W, _ = imgs.shape
  _, q = assert_regime(device, name, N, H, W)
  enc = ops.Encoder(sd, device)
  x = imgs.to(device).contiguous()
  nchw = lambda t: t.permute(0, 3, 1, 2)
  worst = 0.0
  for call_no in range(1, calls + 1):
    c, f = enc(x)
    worst = max(worst, assert_maps(nchw(c), nchw(f), c64, f64, f'encoder {name} forward kernels, call {call_no}', q))
  if other_entries:
    w = {k: torch.from_numpy(np.asarray(sd[k])).float().to(device) for k in train_encoder.PARAMS}
    with torch.no_grad():
      tc, tf = train_encoder.encoder_forward(w, nchw(x))
    worst = max(worst, assert_maps(tc, tf, c64, f64, f'encoder {name} train_encoder.encoder_forward', q))
    del tc, tf
    net = feature_network.ResNet.from_module(_holder(w))
    with torch.no_grad():
      wc, wf = net(nchw(x))
    assert not wc.requires_grad
    worst = max(worst, assert_maps(wc, wf, c64, f64, f'encoder {name} ResNet wrapper under no_grad', q))
  print(f'  encoder {name}: worst fraction of 1e-4 + 1e-4 |ref| used {worst:.3f}')
  return worst


def check_encoder_rejects_small_images(device):
  """15 x 16 and 16 x 15 are below the documented minimum: a Python exception with the library's message, nothing launched"""
  _, sd = cases.encoder_case('min')
  enc = ops.Encoder(sd, device)
  for H, W in ((15, 16), (16, 15)):
    x = torch.full((1, H, W, 3), 0.5, dtype=torch.float32, device=device)
    try:
      enc(x)
    except RuntimeError as e:
      assert 'dyn_encoder' in str(e) and ('16' in str(e) or 'bad argument' in str(e)), f'{H} x {W}: the exception does not carry the library\'s message: {e}'
    else:
      raise AssertionError(f'{H} x {W} images were accepted')
    assert int(_lib.lib().dyn_encoder_workspace_bytes(1, H, W)) == 0
    # the C entry itself, with buffers it could write: refused, buffers untouched
    out = torch.full((2, 4, 4, 32), 7.0, dtype=torch.float32, device=device)
    ws = torch.full((1 << 16,), 7.0, dtype=torch.float32, device=device)
    p = _lib.params('DynEncoderParams', N=1, H=H, W=W, blob=_lib.ptr(enc.blob), images=_lib.ptr(x), coarse=_lib.ptr(out[0]), fine=_lib.ptr(out[1]),
                    workspace=_lib.ptr(ws), workspace_bytes=ws.numel() * 4)
    rc = _lib.lib().dyn_encoder_forward(ctypes.byref(p), _lib.stream_of(x))
    msg = _lib.lib().dyn_last_error().decode()
    assert rc != 0 and 'at least 16 x 16' in msg, (rc, msg)
    _sync(device)
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all()), 'a refused call wrote to its buffers'


def _sync(device):
  if str(device).startswith('cuda'):
    torch.cuda.synchronize()


# ---- B: conditioning of the InstanceNorm statistics ------------------------------------------------------------------------------------
def conditioning_table(tag, got, v32, v64):
  """The _accuracy_table idiom for one map: the kernels' largest and 99th-percentile distance from float64 may be at most twice the fp32 oracle's own
  on the same input, with 1e-4 + 1e-4 |ref| as a floor per element.  Records the fraction used; returns (figures, failures)."""
  g, r32 = parity.cpu(got).double(), v32.double()
  e_our, e_ref = (g - v64).abs(), (r32 - v64).abs()
  floor = 1e-4 + 1e-4 * v64.abs()
  step = max(1, e_our.numel() // 200000)
  q99 = lambda e: float(torch.quantile(e.flatten()[::step], 0.99))
  fig = dict(ours_max=float(e_our.max()), ref_max=float(e_ref.max()), ours_p99=q99(e_our), ref_p99=q99(e_ref))
  fails = []
  for stat in ('max', 'p99'):
    lim = torch.maximum(torch.full_like(floor, 2.0 * fig['ref_' + stat]), floor)
    used = e_our / lim
    u = float(used.max()) if stat == 'max' else q99(used)
    fig['used_' + stat] = u
    parity.record_margin(f'{tag}: error against float64, kernels vs max(twice the fp32 oracle\'s own, 1e-4 + 1e-4 |ref|) ({stat})', torch.tensor([u]), torch.tensor([1.0]))
    if not u <= 1.0:
      fails.append(f'{tag} ({stat}): kernels {fig["ours_" + stat]:.3e} from float64, the fp32 oracle {fig["ref_" + stat]:.3e}: {u:.2f} of the limit')
  print(f'  conditioning [{tag}]: ours max {fig["ours_max"]:.2e} p99 {fig["ours_p99"]:.2e} | fp32 oracle max {fig["ref_max"]:.2e} p99 {fig["ref_p99"]:.2e} | '
        f'used {fig["used_max"]:.2f} (max) {fig["used_p99"]:.2f} (p99)')
  return fig, fails


def check_encoder_conditioning(device, name, shape=None):
  """dim / flat / const frames through the forward-only kernels and the training form's forward, against float64, next to the fp32 oracle.
  Every figure is printed before anything is asserted."""
  from dynibar_amd import train_encoder
  imgs, sd, c64, f64 = reference64(name, shape)
  with torch.no_grad():
    c32, f32 = O.resnet_encoder(O.tdict(sd), imgs.permute(0, 3, 1, 2))
  ratio = None
  with torch.no_grad():  # how ill-conditioned the first norm is on this input
    a = O._conv_reflect(imgs.permute(0, 3, 1, 2).double(), O.tdict(sd)['conv1.weight'].double(), 2, 3).flatten(2)
    ratio = float((a.mean(-1).abs() / a.std(-1).clamp(min=1e-30)).max()) if name != 'const' else float('inf')
  print(f'  conditioning [{name} {tuple(imgs.shape)}]: |mean| / std of a conv1 channel up to {ratio:.3g}')
  x = imgs.to(device).contiguous()
  nchw = lambda t: t.permute(0, 3, 1, 2)
  c, f = ops.Encoder(sd, device)(x)
  w = {k: torch.from_numpy(np.asarray(sd[k])).float().to(device) for k in train_encoder.PARAMS}
  with torch.no_grad():
    tc, tf = train_encoder.encoder_forward(w, nchw(x))
  fails, figs = [], {}
  for tag, got, r32, r64 in ((f'encoder {name} forward kernels coarse', nchw(c), c32, c64), (f'encoder {name} forward kernels fine', nchw(f), f32, f64),
                             (f'encoder {name} training form coarse', tc, c32, c64), (f'encoder {name} training form fine', tf, f32, f64)):
    g = parity.cpu(got)
    assert bool(torch.isfinite(g).all()), f'{tag}: non-finite values (a clamped negative variance?)'
    figs[tag], fl = conditioning_table(tag, g, r32, r64)
    fails += fl
  assert not fails, '\n'.join(fails)
  return figs


# ---- D: the exported helpers ------------------------------------------------------------------------------------------------------------
def _fp(t):
  return ctypes.c_void_p(t.data_ptr())


def _out_hw(H, W, k, stride, pad):
  return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _unfold_reflect(x, k, stride, pad):
  """x [N,H,W,C] -> [N * Ho * Wo, k * k * C] in (ky, kx, c) order: F.unfold of the reflect-padded map, re-ordered from unfold's (c, ky, kx)"""
  N, H, W, C = x.shape
  xp = x.permute(0, 3, 1, 2)
  if pad:
    xp = F.pad(xp, (pad, pad, pad, pad), mode='reflect')
  u = F.unfold(xp, k, stride=stride)  # [N, C * k * k, L]
  L = u.shape[-1]
  return u.reshape(N, C, k * k, L).permute(0, 3, 2, 1).reshape(N * L, k * k * C)


IM2COL_SHAPES = ((16, 16), (19, 25), (37, 50), (74, 49))


def im2col_cases(shapes=IM2COL_SHAPES, channels=(3, 64)):
  return [(k, s, C, H, W) for k, s, C, (H, W) in itertools.product((1, 3, 7), (1, 2), channels, shapes)]


def check_im2col(device, k, stride, C, H, W, N=2, seed=0):
  """dyn_enc_im2col is a copy: bit-exact against F.unfold of the reflect-padded input, padding columns exactly zero"""
  g = torch.Generator().manual_seed(seed + 131 * k + 17 * stride + C + H * W)
  x = torch.randn((N, H, W, C), generator=g)
  pad = k // 2
  Ho, Wo = _out_hw(H, W, k, stride, pad)
  K = k * k * C
  ldc = (K + 3) // 4 * 4 + (4 if C == 64 and k == 3 else 0)  # (one shape with padding columns beyond the rounding, too)
  col = torch.full((N * Ho * Wo, ldc), float('nan'), dtype=torch.float32, device=device)
  xd = x.to(device).contiguous()
  _lib.call('dyn_enc_im2col', _fp(xd), N, H, W, C, k, k, stride, pad, Ho, Wo, _fp(col), ldc, _lib.stream_of(xd))
  got = parity.cpu(col)
  parity.assert_bitexact(got[:, :K], _unfold_reflect(x, k, stride, pad), f'dyn_enc_im2col k={k} stride={stride} C={C} {H}x{W}')
  assert bool((got[:, K:] == 0).all()), 'dyn_enc_im2col: padding columns must be written as zeros'


def check_col2im(device, k, stride, H, W, C=64, N=2, seed=0):
  """dyn_enc_col2im is the adjoint of dyn_enc_im2col: <im2col(x), d> == <x, col2im(d)>, both sums in float64, to 1e-6 of the sum of the absolute
  values of the terms (the kernel adds at most 27 fp32 terms per pixel: 27 * 2^-24 = 1.6e-6 at worst); and it ADDS to din."""
  g = torch.Generator().manual_seed(seed + 131 * k + 17 * stride + H * W)
  pad = k // 2
  Ho, Wo = _out_hw(H, W, k, stride, pad)
  K = k * k * C
  ldc = K
  x = torch.randn((N, H, W, C), generator=g)
  d = torch.randn((N * Ho * Wo, ldc), generator=g)
  base = torch.randn((N, H, W, C), generator=g)
  dd, din = d.to(device).contiguous(), base.clone().to(device).contiguous()
  _lib.call('dyn_enc_col2im', _fp(dd), ldc, N, H, W, C, k, k, stride, pad, Ho, Wo, _fp(din), _lib.stream_of(dd))
  added = parity.cpu(din).double() - base.double()
  col = _unfold_reflect(x, k, stride, pad).double()
  lhs_terms = col * d.double()
  lhs, rhs = float(lhs_terms.sum()), float((x.double() * added).sum())
  scale = float(lhs_terms.abs().sum())
  what = f'dyn_enc_col2im adjoint k={k} stride={stride} {H}x{W}'
  # (subtracting `base` back out in fp32 storage costs 2^-24 |base + sum| per pixel on top of the kernel's own sum; both are inside 27 * 2^-24)
  parity.record_margin(what + ' (<im2col x, d> vs <x, col2im d>)', torch.tensor([abs(lhs - rhs)]), torch.tensor([1e-6 * scale]))
  assert abs(lhs - rhs) <= 1e-6 * scale, f'{what}: {lhs!r} vs {rhs!r}, {abs(lhs - rhs) / scale:.2e} of the terms'
  # element-wise too: the exact adjoint in float64 (autograd of the unfold)
  xr = x.double().requires_grad_(True)
  (_unfold_reflect(xr, k, stride, pad) * d.double()).sum().backward()
  parity.assert_close(added, xr.grad, 2e-6 * float((xr.grad.abs() + base.abs().double()).max()), 0.0, what + ' element-wise, din += (not =)')


IN_HW = (1, 15, 16, 17, 255, 256, 257, 9216)


def _in_reference(x, gamma, beta, res, relu, dy, dtype):
  """instance_norm (+ res) (+ relu) and its autograd in `dtype` on [N, HW, 64] maps -> (y, dx, dres, dgamma, dbeta)"""
  xr = x.to(dtype).requires_grad_(True)
  gr, br = gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)
  rr = res.to(dtype).requires_grad_(True) if res is not None else None
  y = F.instance_norm(xr.permute(0, 2, 1), weight=gr, bias=br, eps=1e-5).permute(0, 2, 1) if x.shape[1] > 1 else \
      ((xr - xr.mean(1, keepdim=True)) * torch.rsqrt(xr.var(1, unbiased=False, keepdim=True) + 1e-5) * gr + br)  # (torch refuses one value per channel)
  if rr is not None:
    y = y + rr
  if relu:
    y = F.relu(y)
  (y * dy.to(dtype)).sum().backward()
  return y.detach(), xr.grad, (rr.grad if rr is not None else None), gr.grad, br.grad


def _run_in_kernels(device, x, gamma, beta, res, relu, dy, dg0, db0):
  N, HW, _ = x.shape
  xd, gd, bd, dyd = (v.to(device).contiguous() for v in (x, gamma, beta, dy))
  rd = res.to(device).contiguous() if res is not None else None
  st = _lib.stream_of(xd)
  stats = torch.zeros((N, 64, 2), dtype=torch.float64, device=device)
  _lib.call('dyn_enc_in_stats', _fp(xd), N, HW, _fp(stats), st)
  y = torch.full_like(xd, float('nan'))
  _lib.call('dyn_enc_in_apply', _fp(xd), _fp(stats), _fp(gd), _fp(bd), _fp(rd) if rd is not None else None, int(relu), N, HW, _fp(y), st)
  sums2 = torch.full((N, 64, 2), float('nan'), dtype=torch.float64, device=device)  # (the entry zeroes it)
  dx = torch.full_like(xd, float('nan'))
  dres = torch.full_like(xd, float('nan')) if rd is not None else None
  dg, db = dg0.to(device).clone(), db0.to(device).clone()
  _lib.call('dyn_enc_in_bwd', _fp(dyd), _fp(y) if relu else None, int(relu), _fp(xd), _fp(stats), _fp(gd), N, HW, _fp(sums2), _fp(dx),
            _fp(dres) if dres is not None else None, _fp(dg), _fp(db), st)
  c = parity.cpu
  return c(y), c(dx), (c(dres) if dres is not None else None), c(dg) - dg0, c(db) - db0, c(stats)


def check_instance_norm(device, HW, N, relu, with_res, seed=0):
  """dyn_enc_in_stats / in_apply / in_bwd against float64 instance_norm autograd; dgamma / dbeta pre-filled (they accumulate).  Limits: the training
  encoder's own (values 1e-4 + 1e-4 |ref|; gradients 3e-5 of the tensor's largest + 1e-4 relative)."""
  g = torch.Generator().manual_seed(seed + 7 * HW + N + 2 * relu + with_res)
  x = torch.randn((N, HW, 64), generator=g) * (0.5 + torch.rand(64, generator=g)) + torch.randn(64, generator=g)
  gamma, beta = 0.5 + torch.rand(64, generator=g), torch.randn(64, generator=g)
  res = torch.randn((N, HW, 64), generator=g) if with_res else None
  dy = torch.randn((N, HW, 64), generator=g)
  dg0, db0 = torch.randn(64, generator=g), torch.randn(64, generator=g)
  y, dx, dres, dg, db, stats = _run_in_kernels(device, x, gamma, beta, res, relu, dy, dg0, db0)
  tag = f'dyn_enc_in HW={HW} N={N} relu={int(relu)} res={int(with_res)}'
  parity.assert_close(stats[..., 0], x.double().sum(1), 1e-5 * float(x.abs().sum(1).max()) + 1e-12, 0.0, tag + ' sum x')
  parity.assert_close(stats[..., 1], x.double().square().sum(1), 0.0, 1e-5, tag + ' sum x^2')
  ry, rdx, rdres, rdg, rdb = _in_reference(x, gamma, beta, res, relu, dy, torch.float64)
  if relu:  # a ReLU argument within rounding of zero is decided by neither side: take the reference gradient with the kernel's decisions
    flips = (y > 0) != (ry > 0)
    assert int(flips.sum()) <= max(1, int(4.5e-5 * y.numel())), f'{tag}: {int(flips.sum())} ReLU decisions differ'
    if bool(flips.any()):
      pre = _in_reference(x, gamma, beta, res, False, dy, torch.float64)[0]
      assert float(pre[flips].abs().max()) < 1e-5 * float(pre.abs().max()), f'{tag}: a ReLU decision differs away from zero'
      dy = dy * (~flips)
      ry, rdx, rdres, rdg, rdb = _in_reference(x, gamma, beta, res, relu, dy, torch.float64)
      y, dx, dres, dg, db, _ = _run_in_kernels(device, x, gamma, beta, res, relu, dy, dg0, db0)
  parity.assert_close(y, ry, 1e-4, 1e-4, tag + ' y')
  for got, ref, nm in ((dx, rdx, 'dx'), (dres, rdres, 'dres'), (dg, rdg, 'dgamma'), (db, rdb, 'dbeta')):
    if ref is None:
      assert got is None
      continue
    scale = float(ref.abs().max())
    # (dgamma / dbeta come back as fp32 (prefill + sum) - prefill: one rounding of |prefill + sum| on top of the kernel's own)
    pre = 2.0 ** -23 * (float(dg0.abs().max()) + scale) if nm in ('dgamma', 'dbeta') else 0.0
    parity.assert_close(got, ref, 3e-5 * scale + 1e-7 + pre, 1e-4, f'{tag} {nm}')


def check_instance_norm_offset(device, HW=9216, N=2):
  """one map with mean 50 and std 0.5 per channel (|mean| / std = 100): the kernels' error against float64 held to twice torch fp32's own, with the
  training encoder's limits as the floor"""
  g = torch.Generator().manual_seed(5)
  x = 50.0 + 0.5 * torch.randn((N, HW, 64), generator=g)
  gamma, beta = 0.5 + torch.rand(64, generator=g), torch.randn(64, generator=g)
  dy = torch.randn((N, HW, 64), generator=g)
  z = torch.zeros(64)
  y, dx, _, dg, db, _ = _run_in_kernels(device, x, gamma, beta, None, False, dy, z, z)
  r64 = _in_reference(x, gamma, beta, None, False, dy, torch.float64)
  r32 = _in_reference(x, gamma, beta, None, False, dy, torch.float32)
  for got, i, nm in ((y, 0, 'y'), (dx, 1, 'dx'), (dg, 3, 'dgamma'), (db, 4, 'dbeta')):
    ref, t32 = r64[i], r32[i].double()
    e_ref = float((t32 - ref).abs().max())
    scale = float(ref.abs().max())
    floor = (1e-4 + 1e-4 * ref.abs()) if nm == 'y' else (3e-5 * scale + 1e-7 + 1e-4 * ref.abs())
    lim = torch.maximum(torch.full_like(ref, 2.0 * e_ref), floor)
    err = (got.double() - ref).abs()
    parity.record_margin(f'dyn_enc_in mean 50 std 0.5 {nm}: kernels vs max(twice torch fp32\'s own error, the training encoder\'s limit)', err, lim)
    print(f'  dyn_enc_in offset map {nm}: ours {float(err.max()):.2e}, torch fp32 {e_ref:.2e}, used {float((err / lim).max()):.2f}')
    assert bool((err <= lim).all()), f'dyn_enc_in offset map {nm}: ours {float(err.max()):.3e} from float64, torch fp32 {e_ref:.3e}'


def check_helper_argument_errors(device):
  """bad arguments return a message through dyn_last_error and launch nothing (every buffer keeps its fill)"""
  L = _lib.lib()
  fill = 3.0
  x = torch.full((1, 16, 16, 64), fill, dtype=torch.float32, device=device)
  col = torch.full((64 * 9 * 64 + 64,), fill, dtype=torch.float32, device=device)  # 8 x 8 rows of a 3x3 / 2 convolution, and slack
  st = _lib.stream_of(x)
  off = lambda t, n: ctypes.c_void_p(t.data_ptr() + 4 * n)
  f64 = torch.full((64 * 2,), fill, dtype=torch.float64, device=device)
  v64 = torch.full((64,), fill, dtype=torch.float32, device=device)
  bad = [
      ('im2col: misaligned patch matrix', lambda: L.dyn_enc_im2col(_fp(x), 1, 16, 16, 64, 3, 3, 2, 1, 8, 8, off(col, 1), 576, st), 'aligned'),
      ('im2col: misaligned map', lambda: L.dyn_enc_im2col(off(x, 1), 1, 15, 16, 64, 3, 3, 2, 1, 8, 8, _fp(col), 576, st), 'aligned'),
      ('im2col: ldc not a multiple of 4', lambda: L.dyn_enc_im2col(_fp(x), 1, 16, 16, 64, 3, 3, 2, 1, 8, 8, _fp(col), 578, st), 'multiple of 4'),
      ('im2col: ldc below K', lambda: L.dyn_enc_im2col(_fp(x), 1, 16, 16, 64, 3, 3, 2, 1, 8, 8, _fp(col), 572, st), 'bad arguments'),
      ('im2col: output size', lambda: L.dyn_enc_im2col(_fp(x), 1, 16, 16, 64, 3, 3, 2, 1, 8, 9, _fp(col), 576, st), 'does not match'),
      ('im2col: pad >= size', lambda: L.dyn_enc_im2col(_fp(x), 1, 3, 16, 64, 7, 7, 1, 3, 3, 16, _fp(col), 3136, st), 'bad geometry'),
      ('col2im: misaligned', lambda: L.dyn_enc_col2im(off(col, 1), 576, 1, 16, 16, 64, 3, 3, 2, 1, 8, 8, _fp(x), st), 'aligned'),
      ('col2im: ldc not a multiple of 4', lambda: L.dyn_enc_col2im(_fp(col), 578, 1, 16, 16, 64, 3, 3, 2, 1, 8, 8, _fp(x), st), 'multiples of 4'),
      ('col2im: output size', lambda: L.dyn_enc_col2im(_fp(col), 576, 1, 16, 16, 64, 3, 3, 2, 1, 9, 8, _fp(x), st), 'does not match'),
      ('in_stats: misaligned', lambda: L.dyn_enc_in_stats(off(x, 1), 1, 16, _fp(f64), st), 'bad arguments'),
      ('in_stats: HW = 0', lambda: L.dyn_enc_in_stats(_fp(x), 1, 0, _fp(f64), st), 'bad arguments'),
      ('in_apply: misaligned output', lambda: L.dyn_enc_in_apply(_fp(x), _fp(f64), _fp(v64), _fp(v64), None, 0, 1, 16, off(col, 1), st), 'bad arguments'),
      ('in_bwd: relu without y', lambda: L.dyn_enc_in_bwd(_fp(x), None, 1, _fp(x), _fp(f64), _fp(v64), 1, 16, _fp(f64), _fp(col), None, _fp(v64), _fp(v64), st), 'bad arguments'),
      ('in_bwd: misaligned dx', lambda: L.dyn_enc_in_bwd(_fp(x), None, 0, _fp(x), _fp(f64), _fp(v64), 1, 16, _fp(f64), off(col, 1), None, _fp(v64), _fp(v64), st), 'alignment'),
  ]
  for what, fn, words in bad:
    rc = fn()
    msg = L.dyn_last_error().decode()
    assert rc != 0, f'{what}: accepted'
    assert words in msg, f'{what}: message {msg!r} does not say {words!r}'
  # the encoder's own entry: workspace too small
  _, sd = cases.encoder_case('min')
  enc = ops.Encoder(sd, device)
  img = torch.full((1, 16, 16, 3), 0.5, dtype=torch.float32, device=device)
  out = torch.full((2, 4, 4, 32), fill, dtype=torch.float32, device=device)
  need = int(L.dyn_encoder_workspace_bytes(1, 16, 16))
  assert need > 0
  ws = torch.full((need // 4,), fill, dtype=torch.float32, device=device)
  p = _lib.params('DynEncoderParams', N=1, H=16, W=16, blob=_lib.ptr(enc.blob), images=_lib.ptr(img), coarse=_lib.ptr(out[0]), fine=_lib.ptr(out[1]),
                  workspace=_lib.ptr(ws), workspace_bytes=need - 4)
  rc = L.dyn_encoder_forward(ctypes.byref(p), st)
  msg = L.dyn_last_error().decode()
  assert rc != 0 and 'workspace too small' in msg, (rc, msg)
  _sync(device)
  for t, nm in ((x, 'map'), (col, 'patch matrix'), (v64, 'vector'), (out, 'encoder outputs'), (ws, 'workspace')):
    assert bool((t == fill).all()), f'a refused call wrote to the {nm}'
  assert bool((f64 == fill).all()), 'a refused call wrote to the statistics table'
