"""The row kernels of csrc/dyn_train.hip one entry point at a time, called through the C ABI, parameterised by device like tests/parity.py
(a real MI355X under -m gpu, CPU tensors under the wave-level emulator).

Two families per check:

  (a) exact.  Inputs are small dyadic rationals (multiples of 1/8 or coarser), chosen so that every product and every partial sum of the
      float64 result is representable in fp32: the order of summation, of shuffles and of atomics cannot matter, and every element-wise
      output AND every reduction (dbias, dseg, ds, dW, dw, absmax, nvalid, the colsum_reduce sums) is asserted EQUAL.  The precondition is
      asserted on the float64 reference alone, before the kernel runs (`_exact`, `_sum_exact`): ref == ref.float().double() and, per sum,
      sum |terms| / (lsb of the smallest term) < 2^24.  Outputs a kernel must fill start as NaN; padding columns and neighbours of a
      wider matrix start from PAD and are asserted unchanged.

  (b) accuracy, for everything through expf / expm1f / sincosf / sigmoid / rsqrt / a division: standard-normal inputs, limit =
      2 x (largest error of a plain fp32 torch restatement of the reference's formula against its float64 twin on the same inputs)
      + 2e-6 of the output's magnitude (the floor of tests/objective_cases.py); for a cancelling reduction the magnitude is the float64
      sum of the absolute terms.  The limit is not chosen for the kernel.  The restatements follow the reference's formulas
      (mlp_network.py, render_ray.py as restated in oracle/ibr_oracle.py), never the kernel code; tests/test_train_rows_cpu.py pins them
      against autograd through the oracle / torch.nn.functional.

Entry point -> check:
  dyn_train_act_bwd                         check_act_bwd, check_act_bwd_tall
  dyn_train_absmax                          check_absmax
  dyn_train_colsum_reduce                   check_colsum_reduce
  dyn_train_rowscale, dyn_train_rowscale_bwd  check_rowscale
  dyn_train_rowscale_act_bwd                check_rowscale_act_bwd
  dyn_train_vis_split, dyn_train_vis_split_bwd  check_vis_split
  dyn_train_vis_split_act_bwd               check_vis_split_act_bwd
  dyn_train_rowdot, dyn_train_outer_act_bwd  check_rowdot_outer
  dyn_train_meanvar(_bwd)                   check_meanvar
  dyn_train_view_weights(_bwd)              check_view_weights
  dyn_train_layernorm(_bwd)                 check_layernorm
  dyn_train_blend(_bwd)                     check_blend
  dyn_train_dynamic_head(_bwd)              check_dynamic_head
  dyn_train_add_table                       check_add_table
  dyn_train_embed(_bwd)                     check_embed
  dyn_train_dynamic_embed                   check_dynamic_embed
  dyn_train_static_embed                    check_static_embed
  dyn_train_build_f(_bwd)                   check_build_f
  dyn_train_zero_tail                       check_zero_tail
  argument errors                           check_argument_errors
"""
import ctypes

import torch
import torch.nn.functional as F

from oracle import ibr_oracle as O
from parity import assert_bitexact, assert_close, cpu, record_margin

PAD = 77.0      # what padding columns / neighbouring columns hold before a launch
SPAN = 256      # rows per lane group of the fused backward kernels (TR_FUSE_SPAN)
BLOCK = 2048    # rows per block of the 128-column fused kernels
NAN = float('nan')


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
DRY = [False]   # tests/test_train_rows_cpu.py: walk every case for its references and preconditions alone -- no library, no launch, no comparison
DRY_ERR32 = {}  # (check, output) -> the largest error of the fp32 restatement seen in a dry walk


def _api():
  if DRY[0]:
    return (lambda t, off=0: None), (lambda t: None), (lambda *a: None)
  from dynibar_amd import train_static as TS
  from dynibar_amd._lib import call
  keep = []

  def p(t, off=0):
    keep.append(t)  # a pointer does not keep its tensor alive: temporaries handed to a launch live as long as the check's `_p`
    return TS._p(t, off)
  return p, TS.stream_of, call


def gen(seed):
  return torch.Generator().manual_seed(seed)


def dyadic(g, *shape, den=8, lim=4, lo=None):
  """random multiples of 1/den in [-lim, lim] (or [lo, lim]), float64"""
  a = int((-lim if lo is None else lo) * den)
  return torch.randint(a, int(lim * den) + 1, shape, generator=g).double() / den


def _lsb(t):
  """largest power of two that divides every non-zero element (the elements are multiples of 2^-40 below 2^20: asserted)"""
  s = t.double().reshape(-1) * 2.0 ** 40
  q = s.round().long()
  assert bool((q.double() == s).all()) and bool((s.abs() < 2.0 ** 60).all()), 'terms are not dyadic rationals of the expected range'
  q = q[q != 0].abs()
  if q.numel() == 0:
    return 1.0
  return float((q & -q).min()) / 2.0 ** 40


def _exact(ref, what):
  """precondition (a): the float64 result is an fp32 number"""
  assert torch.equal(ref, ref.float().double()), f'{what}: the float64 reference is not representable in fp32 (test input bug)'
  return ref


def _sum_exact(terms, dim, what):
  """precondition (a) of a sum: sum |terms| / lsb < 2^24 along `dim`, so no partial sum in any order can round"""
  lsb = _lsb(terms)
  worst = float(terms.abs().sum(dim).max()) / lsb
  assert worst < 2.0 ** 24, f'{what}: partial sums need {worst:.3g} > 2^24 steps of {lsb:g} (test input bug)'
  return _exact(terms.sum(dim), what)


def mat(x, ld, device, off=0, guard=0):
  """[rows, cols] values inside a [rows, ld] buffer whose other columns hold PAD, `off` floats into its allocation, followed by `guard` rows of
  NaN (inside the allocation: a kernel that reads rows past the end and lets them into a result shows it) -> (flat, view)"""
  rows, cols = x.shape
  flat = torch.full((off + (rows + guard) * ld,), PAD, dtype=torch.float32)
  flat[off + rows * ld:] = NAN
  flat[off:off + rows * ld].view(rows, ld)[:, :cols] = x.float()
  flat = flat.to(device)
  return flat, flat[off:off + rows * ld].view(rows, ld)


def dv(x, device):
  return x.float().contiguous().to(device)


def assert_pad(view, cols, what):
  if DRY[0]:
    return
  pad = cpu(view)[:, cols:]
  assert bool((pad == PAD).all()), f'{what}: {int((pad != PAD).sum())} padding / neighbour elements were overwritten'


def assert_equal(got, ref, what):
  """bit equality against the float64 reference (which precondition (a) made an fp32 number); NaN (an element never written) fails"""
  if DRY[0]:
    return
  got = cpu(got)
  assert not bool(torch.isnan(got).any()), f'{what}: {int(torch.isnan(got).sum())}/{got.numel()} elements were never written'
  assert_bitexact(got, ref.float().reshape(got.shape), what)


def limit_of(v32, v64, magnitude=None):
  """family (b): 2 x the fp32 restatement's largest error + 2e-6 of the magnitude"""
  mag = float(v64.abs().max()) if magnitude is None else float(magnitude)
  return 2.0 * float((v32.double() - v64).abs().max()) + 2e-6 * mag


def assert_within(got, v32, v64, what, magnitude=None):
  if DRY[0]:
    key = (what.split()[0], what.split()[-1])
    DRY_ERR32[key] = max(DRY_ERR32.get(key, 0.0), float((v32.double() - v64).abs().max()))
    return
  got = cpu(got).double().reshape(v64.shape)
  assert not bool(torch.isnan(got).any()), f'{what}: NaN in the output'
  lim = limit_of(v32, v64, magnitude)
  err = (got - v64).abs()
  if lim == 0.0:
    assert float(err.max()) == 0.0, f'{what}: max err {float(err.max()):.3e} where the reference is exact'
    return
  assert_close(got, v64, lim, 0.0, what)


def leaf(t, dt):
  return t.detach().clone().to(dt).requires_grad_(True)


def dact(y, act):
  """derivative of the activation from its saved OUTPUT: ELU' = y + 1 below zero (F.elu: alpha = 1), ReLU' = 0"""
  one = torch.ones_like(y)
  return one if act == 0 else torch.where(y > 0, one, y + 1 if act == 1 else torch.zeros_like(y))


def round_up(n, m):
  return (n + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------------
# dyn_train_act_bwd
# ---------------------------------------------------------------------------------------------------------------------
def act_bwd_reference(dY, Y, act, seg):
  dZ = dY * dact(Y, act)
  return dZ, (dZ.view(-1, seg, dZ.shape[1]) if seg else None)


def act_bwd_inputs(rows, cols, seed, coarse=False):
  g = gen(seed)
  if coarse:  # the tall case: 2^20 rows of {-1, 0, 1}
    dY = torch.randint(-1, 2, (rows, cols), generator=g).double()
    Y = torch.randint(-1, 2, (rows, cols), generator=g).double()
  else:
    dY, Y = dyadic(g, rows, cols, den=8, lim=4), dyadic(g, rows, cols, den=8, lim=1)
  dY[-1, -1], Y[-1, -1] = (2.0 if coarse else 8.0), 1.0  # the largest |dZ| is the last element of the last row
  return dY, Y


def check_act_bwd(device, rows, cols, act, ld=None, bias=True, seg=0, ld_seg=None, off=0, seed=0, coarse=False):
  """dZ = dY act'(Y) in place, dbias += column sums, dseg = sums over the seg rows of a point, *absmax = max |dZ|: all equal"""
  _p, stream_of, call = _api()
  ld = cols if ld is None else ld
  what = f'act_bwd rows={rows} cols={cols} ld={ld} act={act} bias={bias} seg={seg} ld_seg={ld_seg} off={off}'
  dY, Y = act_bwd_inputs(rows, cols, seed, coarse)
  dZ, segs = act_bwd_reference(dY, Y, act, seg)
  _exact(dZ, what)
  b0 = dyadic(gen(seed + 1), cols, den=8, lim=2)
  dseg_ref = _sum_exact(segs, 1, what + ' dseg') if seg else None
  dbias_ref = _sum_exact(torch.cat([dZ, b0[None]]), 0, what + ' dbias')  # (dbias accumulates: it starts from b0)
  amax_ref = dZ.abs().max()
  fdy, vdy = mat(dY, ld, device, off)
  fy, vy = mat(Y, ld, device, off)
  dbias = dv(b0, device) if bias else None
  absmax = torch.zeros(1, device=device)
  dseg = None
  if seg:
    ld_seg = cols if ld_seg is None else ld_seg
    fseg, dseg = mat(torch.full((rows // seg, cols), NAN), ld_seg, device)
  call('dyn_train_act_bwd', _p(fdy, off), _p(fy, off) if act else None, rows, cols, ld, ld, act, _p(dbias) if bias else None, seg,
       _p(fseg) if seg else None, ld_seg or 0, _p(absmax), stream_of(fdy))
  assert_equal(vdy[:, :cols], dZ, what + ' dZ')
  assert_pad(vdy, cols, what + ' dY')
  if bias:
    assert_equal(dbias, dbias_ref, what + ' dbias')
  if seg:
    assert_equal(dseg[:, :cols], dseg_ref, what + ' dseg')
    assert_pad(dseg, cols, what + ' dseg')
  assert_equal(absmax, amax_ref.reshape(1), what + ' absmax')


def act_bwd_cases():
  """(rows, cols, act, kwargs).  16-byte form: 16 <= cols <= 256, cols % 4 == 0, aligned; L = cols / 4 lanes per row, G = 256 / L lane groups of
  span = 256 / G rows (whole segments): rows 1, span - 1, span, span + 1, one past a block.  Scalar form: runs of 256 rows, 256 / ct runs per block."""
  out = []
  n = 0
  for cols in (16, 24, 64, 128, 256):
    L = cols // 4
    G = 256 // L
    span = 256 // G
    for rows in (1, span - 1, span, span + 1, G * span + 1):
      for act in (0, 1, 2):
        out.append((rows, cols, act, dict(bias=n % 4 != 3)))
        n += 1
  for cols, ld in ((12, 12), (35, 35), (129, 132), (260, 260)):
    ct = 32 if cols <= 32 else 64 if cols <= 64 else 128 if cols <= 128 else 256
    for rows in (1, 255, 256, 257, 256 * (256 // ct) + 1):
      for act in (0, 1, 2):
        out.append((rows, cols, act, dict(ld=ld, bias=n % 4 != 3)))
        n += 1
  # padding columns in the 16-byte form (ld > cols, both multiples of four)
  for act in (0, 1, 2):
    out.append((37, 64, act, dict(ld=72)))
  # segment sums: seg 3 and 10, 16-byte and scalar forms, span rounded up to whole segments
  for seg in (3, 10):
    for cols, kw in ((16, {}), (24, {}), (128, dict(ld=136)), (64, dict(ld_seg=66)), (12, {}), (129, dict(ld=132, ld_seg=129))):
      for rows in (seg, round_up(257, seg), round_up(2049, seg) if cols in (12, 16) else round_up(300, seg)):
        out.append((rows, cols, n % 3, dict(seg=seg, **kw)))
        n += 1
  # fall-backs to the scalar form that must still be right: a base one float off 16-byte alignment, ld_seg not a multiple of four
  out.append((261, 64, 1, dict(off=1)))
  out.append((261, 64, 2, dict(off=1, ld=68)))
  out.append((260, 64, 1, dict(seg=10, ld_seg=65)))
  return out


def check_act_bwd_tall(device):
  """rows >= 2^20 changes the rows per block of both forms (2048 / G per lane group, runs of 1024): 2^20 + 5 rows (a multiple of seg = 3) of
  {-1, 0, 1} with ReLU, 16 columns (16-byte form, span 33) and 3 columns (scalar form)"""
  rows = (1 << 20) + 5
  check_act_bwd(device, rows, 16, 2, seg=3, seed=5, coarse=True)
  check_act_bwd(device, rows, 3, 2, seg=3, seed=6, coarse=True)


# ---------------------------------------------------------------------------------------------------------------------
# dyn_train_absmax, dyn_train_colsum_reduce
# ---------------------------------------------------------------------------------------------------------------------
def check_absmax(device, rows, cols, ld=None, off=0, init=0.0, seed=0):
  """all three forms (16-byte: contiguous, rows * cols % 4 == 0, aligned; flat: contiguous; window: ld > cols with poison beyond cols);
  the largest element is the last of the last row; *absmax only ever grows (an initial value above the data stays)"""
  _p, stream_of, call = _api()
  ld = cols if ld is None else ld
  what = f'absmax rows={rows} cols={cols} ld={ld} off={off} init={init}'
  x = dyadic(gen(seed), rows, cols, den=8, lim=4)
  x[-1, -1] = -9.0
  flat = torch.full((off + rows * ld,), 100.0)
  flat[off:].view(rows, ld)[:, :cols] = x.float()
  flat = flat.to(device)
  am = torch.full((1,), init, device=device)
  call('dyn_train_absmax', _p(flat, off), rows, cols, ld, _p(am), stream_of(flat))
  assert_equal(am, torch.tensor([max(init, 9.0)]).double(), what)


def absmax_cases():
  return [dict(rows=1, cols=1), dict(rows=1, cols=1, init=20.0), dict(rows=7, cols=4), dict(rows=3, cols=3), dict(rows=5, cols=4, off=1),
          dict(rows=1030, cols=128), dict(rows=4099, cols=35), dict(rows=1030, cols=128, init=20.0),
          dict(rows=1, cols=5, ld=8), dict(rows=67, cols=35, ld=36), dict(rows=1031, cols=70, ld=72), dict(rows=300, cols=128, ld=136),
          dict(rows=131, cols=260, ld=264), dict(rows=67, cols=35, ld=36, init=20.0)]


def check_colsum_reduce(device, tiles, N, ld=None, bias=True, seed=0):
  """dbias[n] += sum over tiles of part[tile, n]; *absmax = max(*absmax, amax_part[...]): equal (dyadic partial sums)"""
  _p, stream_of, call = _api()
  ld = N if ld is None else ld
  what = f'colsum_reduce tiles={tiles} N={N} ld={ld} bias={bias}'
  g = gen(seed)
  part = dyadic(g, tiles, N, den=8, lim=4)
  b0 = dyadic(g, N, den=8, lim=2)
  n_amax = tiles * 3 + 1
  apart = dyadic(g, n_amax, den=8, lim=4, lo=0)
  apart[-1] = 6.5
  ref = _sum_exact(torch.cat([part, b0[None]]), 0, what)
  fpart, vpart = mat(part, ld, device)
  dbias = dv(b0, device)
  am = torch.full((1,), 0.25, device=device)
  call('dyn_train_colsum_reduce', _p(fpart), tiles, N, ld, _p(dbias) if bias else None, _p(dv(apart, device)), n_amax, _p(am), stream_of(fpart))
  assert_equal(dbias, ref if bias else b0, what + ' dbias')
  assert_equal(am, torch.tensor([6.5]).double(), what + ' absmax')


def colsum_reduce_cases():
  out = [dict(tiles=t, N=n) for t in (1, 63, 64, 65, 300) for n in (5, 64, 129)]
  return out + [dict(tiles=65, N=129, ld=132), dict(tiles=300, N=64, ld=72), dict(tiles=65, N=64, bias=False)]


# ---------------------------------------------------------------------------------------------------------------------
# dyn_train_rowscale, dyn_train_rowscale_bwd (exported, no caller), dyn_train_rowscale_act_bwd
# ---------------------------------------------------------------------------------------------------------------------
def check_rowscale(device, N, C, ld=None, accumulate=0, ds_accumulate=0, seed=0):
  """y = x s[row]; dx (+)= dy s[row]; ds[row] (+)= <dy[row], x[row]>.  16-byte forms: C / 4 a power of two (backward: up to 64 lanes),
  aligned; the others by element / one wave per row.  s and ds are columns of wider matrices (strides 3 and 2)."""
  _p, stream_of, call = _api()
  ld = C if ld is None else ld
  what = f'rowscale N={N} C={C} ld={ld} acc={accumulate}/{ds_accumulate}'
  g = gen(seed)
  x, dy, s = dyadic(g, N, C, den=8, lim=2), dyadic(g, N, C, den=8, lim=2), dyadic(g, N, den=8, lim=2)
  dx0, ds0 = dyadic(g, N, C, den=8, lim=2), dyadic(g, N, den=8, lim=2)
  y_ref = _exact(x * s[:, None], what)
  dx_ref = _exact(dy * s[:, None] + (dx0 if accumulate else 0), what)
  ds_ref = _sum_exact(torch.cat([dy * x, ds0[:, None] * (1 if ds_accumulate else 0)], 1), 1, what + ' ds')
  fx, vx = mat(x, ld, device)
  fs, vs = mat(s[:, None], 3, device)
  fy, vy = mat(torch.full((N, C), NAN), ld, device)
  call('dyn_train_rowscale', _p(fx), ld, _p(fs), 3, N, C, _p(fy), ld, stream_of(fx))
  assert_equal(vy[:, :C], y_ref, what + ' y')
  assert_pad(vy, C, what + ' y')
  fdy, _ = mat(dy, ld, device)
  fdx, vdx = mat(dx0 if accumulate else torch.full((N, C), NAN), ld, device)
  fds, vds = mat((ds0 if ds_accumulate else torch.full((N,), NAN))[:, None], 2, device)
  call('dyn_train_rowscale_bwd', _p(fdy), ld, _p(fx), ld, _p(fs), 3, N, C, _p(fdx), ld, accumulate, _p(fds), 2, ds_accumulate, stream_of(fx))
  assert_equal(vdx[:, :C], dx_ref, what + ' dx')
  assert_pad(vdx, C, what + ' dx')
  assert_equal(vds[:, 0], ds_ref, what + ' ds')
  assert_pad(vds, 1, what + ' ds')


def rowscale_cases():
  """C 16 / 128 / 256: both 16-byte forms; 24 (6 lanes: not a power of two), 35: element forms; 512: 16-byte forward, wave-per-row backward.
  In the 16-byte backward form N * C / 4 is no multiple of 64, so the last wave is partly dead (its lanes clamp to row N - 1)."""
  out = []
  n = 0
  for C, ld in ((16, 16), (16, 20), (24, 24), (35, 35), (35, 36), (128, 128), (128, 136), (256, 256), (512, 512)):
    for N in (1, 5, 67, 261):
      out.append(dict(N=N, C=C, ld=ld, accumulate=n & 1, ds_accumulate=(n >> 1) & 1))
      n += 1
  return out


FUSED_N = (1, 255, 256, 257, 511, 513, 2047, 2048, 2049, 2048 + 259)


def check_rowscale_act_bwd(device, N, act, ds_accumulate, bias=True, seed=0):
  """dx = (dx + dy s[row]) act'(x), ds[row] (+)= <dy[row], x[row]>, dbias += column sums of dx, *absmax = max |dx|; 128 columns, ld_dx 136"""
  _p, stream_of, call = _api()
  what = f'rowscale_act_bwd N={N} act={act} ds_acc={ds_accumulate} bias={bias}'
  g = gen(seed)
  x, dy, s = dyadic(g, N, 128, den=8, lim=1), dyadic(g, N, 128, den=8, lim=2), dyadic(g, N, den=8, lim=2)
  dx0, ds0, b0 = dyadic(g, N, 128, den=8, lim=2), dyadic(g, N, den=8, lim=2), dyadic(g, 128, den=8, lim=2)
  dx0[-1, -1], dy[-1, -1], s[-1], x[-1, -1] = 8.0, 2.0, 2.0, 1.0  # the largest |dx| (12) is the last element of the last row
  dx_ref = _exact((dx0 + dy * s[:, None]) * dact(x, act), what)
  ds_ref = _sum_exact(torch.cat([dy * x, ds0[:, None] * (1 if ds_accumulate else 0)], 1), 1, what + ' ds')
  db_ref = _sum_exact(torch.cat([dx_ref, b0[None]]), 0, what + ' dbias')
  fdy, _ = mat(dy, 132, device)
  fx, _ = mat(x, 128, device)
  fs, _ = mat(s[:, None], 3, device)
  fdx, vdx = mat(dx0, 136, device)
  fds, vds = mat((ds0 if ds_accumulate else torch.full((N,), NAN))[:, None], 2, device)
  dbias, am = dv(b0, device), torch.zeros(1, device=device)
  call('dyn_train_rowscale_act_bwd', _p(fdy), 132, _p(fx), 128, _p(fs), 3, N, _p(fdx), 136, _p(fds), 2, ds_accumulate, act,
       _p(dbias) if bias else None, _p(am), stream_of(fx))
  assert_equal(vdx[:, :128], dx_ref, what + ' dx')
  assert_pad(vdx, 128, what + ' dx columns 128..135')
  assert_equal(vds[:, 0], ds_ref, what + ' ds')
  assert_pad(vds, 1, what + ' ds')
  assert_equal(dbias, db_ref if bias else b0, what + ' dbias')
  assert_equal(am, dx_ref.abs().max().reshape(1), what + ' absmax')


def rowscale_act_bwd_cases(act):
  return [dict(N=N, act=act, ds_accumulate=acc, bias=not (acc == 0 and i == 4)) for i, N in enumerate(FUSED_N) for acc in (0, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# the visibility split: dyn_train_vis_split, dyn_train_vis_split_bwd (exported, no caller), dyn_train_vis_split_act_bwd
# (mlp_network.py:466-469: x_res, vis = split(x_vis); vis = sigmoid(vis) mask; x = x + x_res)
# ---------------------------------------------------------------------------------------------------------------------
def vis_split_restatement(x1, xv, mask, dt):
  x1, xv, mask = x1.to(dt), xv.to(dt), mask.to(dt)
  return x1 + xv[:, :128], torch.sigmoid(xv[:, 128]) * mask


def vis_split_bwd_restatement(dx2, dvis0, xv, mask, dt):
  """gradient of the split w.r.t. xv [N, 129] by autograd"""
  dx2, dvis0, mask = dx2.to(dt), dvis0.to(dt), mask.to(dt)
  z = leaf(xv, dt)
  x2, vis = vis_split_restatement(torch.zeros_like(dx2), z, mask, dt)
  ((x2 * dx2).sum() + (vis * dvis0).sum()).backward()
  return z.grad


def check_vis_split(device, N, ray_diff, seed=0):
  """forward (x2 equal, vis0 within the family (b) limit, the [ray_diff | 0 0 0] tail of the 136-column layout equal, column 128 untouched)
  and the unfused backward dxv = [dx2 | dvis0 mask sigmoid'(xv[:, 128])]"""
  _p, stream_of, call = _api()
  what = f'vis_split N={N} ray_diff={ray_diff}'
  g = gen(seed)
  x1, xv = dyadic(g, N, 128, den=8, lim=4), torch.cat([dyadic(g, N, 128, den=8, lim=4), torch.randn(N, 1, generator=g).double() * 2], 1)
  mask = torch.randint(0, 2, (N,), generator=g).double()
  rd = dyadic(g, N, 4, den=8, lim=1)
  x2_ref, vis_ref = vis_split_restatement(x1, xv, mask, torch.float64)
  _, vis32 = vis_split_restatement(x1, xv, mask, torch.float32)
  _exact(x2_ref, what)
  fx1, _ = mat(x1, 128, device)
  fxv, _ = mat(xv, 132, device)
  fx2, vx2 = mat(torch.full((N, 128), NAN), 136, device)
  vis0 = torch.full((N,), NAN, device=device)
  m_d = dv(mask, device)
  call('dyn_train_vis_split', _p(fx1), 128, _p(fxv), 132, _p(m_d), _p(dv(rd, device)) if ray_diff else None, N, _p(fx2), 136, _p(vis0), stream_of(fx1))
  assert_equal(vx2[:, :128], x2_ref, what + ' x2')
  assert_within(vis0, vis32, vis_ref, what + ' vis0')
  if ray_diff:
    assert_pad(vx2[:, 128:129], 0, what + ' column 128')
    assert_equal(vx2[:, 129:133], rd, what + ' ray_diff columns')
    assert_equal(vx2[:, 133:136], torch.zeros(N, 3).double(), what + ' zero columns')
  else:
    assert_pad(vx2, 128, what + ' x2')
  # backward
  dx2, dvis0 = dyadic(g, N, 128, den=8, lim=4), torch.randn(N, generator=g).double()
  ref = vis_split_bwd_restatement(dx2, dvis0, xv, mask, torch.float64)
  r32 = vis_split_bwd_restatement(dx2, dvis0, xv, mask, torch.float32)
  fdx2, _ = mat(dx2, 136, device)
  fdxv, vdxv = mat(torch.full((N, 129), NAN), 132, device)
  call('dyn_train_vis_split_bwd', _p(fdx2), 136, _p(dv(dvis0, device)), _p(fxv), 132, _p(m_d), N, _p(fdxv), 132, stream_of(fx1))
  assert_equal(vdxv[:, :128], dx2, what + ' dxv[:, :128]')
  assert_within(vdxv[:, 128], r32[:, 128], ref[:, 128], what + ' dxv[:, 128]')
  assert_pad(vdxv, 129, what + ' dxv')


def check_vis_split_act_bwd(device, N, fused, bias=True, exact128=True, seed=0):
  """dxv[:, :128] = dx2 ELU'(xv), dxv[:, 128] = dvis0 mask sigmoid'(xv128) ELU'(xv128), dbias[129] += column sums, *absmax = max |dxv|.
  fused: dx2 += dxs vis0[row] first (written back) and dvis0[row] = <dxs[row], x2[row]>.
  exact128: xv[:, 128] = 0 (sigmoid = 1/2, sigmoid' = 1/4, ELU' = 1: exact), so column 128, dbias[128] and absmax are EQUAL too, and the
  largest |dxv| of the matrix is column 128 of the last row.  Otherwise column 128 is standard normal: family (b), and absmax must equal the
  largest magnitude of what the kernel itself wrote."""
  _p, stream_of, call = _api()
  what = f'vis_split_act_bwd N={N} fused={fused} bias={bias} exact128={exact128}'
  g = gen(seed)
  dx2 = dyadic(g, N, 128, den=8, lim=2)
  xv = torch.cat([dyadic(g, N, 128, den=8, lim=1), torch.zeros(N, 1).double() if exact128 else torch.randn(N, 1, generator=g).double() * 2], 1)
  mask = torch.randint(0, 2, (N,), generator=g).double()
  mask[-1] = 1.0
  b0 = dyadic(g, 129, den=8, lim=2)
  if fused:
    dxs, x2, vis0 = dyadic(g, N, 128, den=8, lim=2), dyadic(g, N, 128, den=8, lim=1), dyadic(g, N, den=8, lim=1, lo=0)
    if exact128:
      dxs[-1], x2[-1] = 2.0, 1.0  # <dxs, x2> = 256 in the last row: column 128 = 64, above everything else
    dx2_new = _exact(dx2 + dxs * vis0[:, None], what)
    dvis0 = _sum_exact(dxs * x2, 1, what + ' dvis0')
  else:
    dvis0 = dyadic(g, N, den=8, lim=4) if exact128 else torch.randn(N, generator=g).double()
    if exact128:
      dvis0[-1] = 64.0  # column 128 of the last row = 16
    dx2_new = dx2
  # the split's gradient by autograd, then ELU' of vis_fc.2 from its saved OUTPUT xv (y > 0 ? 1 : y + 1)
  r64 = vis_split_bwd_restatement(dx2_new, dvis0, xv, mask, torch.float64) * dact(xv, 1)
  r32 = vis_split_bwd_restatement(dx2_new, dvis0, xv, mask, torch.float32) * dact(xv.float(), 1)
  main, col, col32 = _exact(r64[:, :128], what), r64[:, 128], r32[:, 128]
  db_main = _sum_exact(torch.cat([main, b0[None, :128]]), 0, what + ' dbias')
  fdx2, vdx2 = mat(dx2, 136, device)
  fxv, _ = mat(xv, 132, device)
  fdxv, vdxv = mat(torch.full((N, 129), NAN), 132, device)
  dbias, am, m_d = dv(b0, device), torch.zeros(1, device=device), dv(mask, device)
  if fused:
    fdxs, _ = mat(dxs, 128, device)
    fx2, _ = mat(x2, 136, device)
    v_d = dv(vis0, device)
  call('dyn_train_vis_split_act_bwd', _p(fdx2), 136, None if fused else _p(dv(dvis0, device)), _p(fxv), 132, _p(m_d), N, _p(fdxv), 132,
       _p(dbias) if bias else None, _p(am), _p(fdxs) if fused else None, 128 if fused else 0, _p(fx2) if fused else None, 136 if fused else 0,
       _p(v_d) if fused else None, stream_of(fdx2))
  assert_equal(vdxv[:, :128], main, what + ' dxv[:, :128]')
  assert_pad(vdxv, 129, what + ' dxv')
  assert_equal(vdx2[:, :128], dx2_new, what + ' dx2 (written back only when fused)')
  assert_pad(vdx2, 128, what + ' dx2 columns 128..135')
  if exact128:
    _exact(col, what)
    assert_equal(vdxv[:, 128], col, what + ' dxv[:, 128]')
    assert float(col[-1].abs()) > float(main.abs().max()), 'test input bug: column 128 must hold the largest magnitude'
    assert_equal(am, torch.maximum(col.abs().max(), main.abs().max()).reshape(1), what + ' absmax')
    if bias:
      assert_equal(dbias[:128], db_main, what + ' dbias[:128]')
      assert_equal(dbias[128:], _sum_exact(torch.cat([col, b0[128:]]), 0, what + ' dbias[128]').reshape(1), what + ' dbias[128]')
  else:
    assert_within(vdxv[:, 128], col32, col, what + ' dxv[:, 128]')
    if not DRY[0]:
      assert_bitexact(am, cpu(vdxv[:, :129]).abs().max().reshape(1), what + ' absmax = the largest magnitude written')
    if bias:
      assert_equal(dbias[:128], db_main, what + ' dbias[:128]')
      assert_within(dbias[128:] - float(b0[128]), col32.sum().reshape(1), col.sum().reshape(1), what + ' dbias[128]',
                    magnitude=float(col.abs().sum()) + abs(float(b0[128])))
  if not bias:
    assert_equal(dbias, b0, what + ' dbias untouched')


def vis_split_act_bwd_cases(fused):
  out = [dict(N=N, fused=fused, bias=not (i == 3)) for i, N in enumerate(FUSED_N)]
  return out + [dict(N=N, fused=fused, exact128=False, bias=N != 257) for N in (1, 257, 2049)]


# ---------------------------------------------------------------------------------------------------------------------
# a Linear with ONE output as row kernels: dyn_train_rowdot, dyn_train_outer_act_bwd
# ---------------------------------------------------------------------------------------------------------------------
def check_rowdot_outer(device, N, C, act, bias=True, dW=True, seed=0):
  """y[row] = <X[row], w> + b;  dX = dz[row] w act'(Y), dbias += column sums, dW += sum_rows dz Y, *absmax = max |dX|: all equal.
  y and dz are columns of wider matrices (strides 2 and 3), X / Y / dX have padding columns."""
  _p, stream_of, call = _api()
  what = f'rowdot/outer N={N} C={C} act={act} bias={bias} dW={dW}'
  g = gen(seed)
  den = 8 if N <= 3000 else 2  # (column sums over tens of thousands of rows: coarser values keep them below 2^24 steps)
  X, w, b = dyadic(g, N, C, den=8, lim=2), dyadic(g, C, den=den, lim=2), dyadic(g, 1, den=8, lim=2)
  y_ref = _sum_exact(torch.cat([X * w, (b if bias else b * 0).expand(N, 1)], 1), 1, what + ' y')
  fX, _ = mat(X, C + 4, device)
  w_d = dv(w, device)
  fy, vy = mat(torch.full((N, 1), NAN), 2, device)
  call('dyn_train_rowdot', _p(fX), C + 4, _p(w_d), _p(dv(b, device)) if bias else None, N, C, _p(fy), 2, stream_of(fX))
  assert_equal(vy[:, 0], y_ref, what + ' y')
  assert_pad(vy, 1, what + ' y')
  # backward through the activation of the layer in front (Y: its saved output)
  Y, dz = dyadic(g, N, C, den=den, lim=1), dyadic(g, N, den=den, lim=2 if den == 8 else 1)
  b0, w0 = dyadic(g, C, den=8, lim=2), dyadic(g, C, den=8, lim=2)
  dz[-1], Y[-1, -1] = 4.0, 1.0
  w = w.clone()
  w[-1] = 3.0  # the largest |dX| (12) is the last element of the last row
  w_d = dv(w, device)
  dX_ref = _exact(dz[:, None] * w[None] * dact(Y, act), what)
  db_ref = _sum_exact(torch.cat([dX_ref, b0[None]]), 0, what + ' dbias')
  dW_ref = _sum_exact(torch.cat([dz[:, None] * Y, w0[None]]), 0, what + ' dW')
  fY, _ = mat(Y, C + 8, device)
  fdz, _ = mat(dz[:, None], 3, device)
  fdX, vdX = mat(torch.full((N, C), NAN), C + 4, device)
  dbias, dWd, am = dv(b0, device), dv(w0, device), torch.zeros(1, device=device)
  use_dW = dW and act != 0
  call('dyn_train_outer_act_bwd', _p(fdz), 3, _p(w_d), _p(fY) if act else None, C + 8, N, C, act, _p(fdX), C + 4, _p(dbias) if bias else None, _p(am),
       _p(dWd) if use_dW else None, stream_of(fX))
  assert_equal(vdX[:, :C], dX_ref, what + ' dX')
  assert_pad(vdX, C, what + ' dX')
  assert_equal(dbias, db_ref if bias else b0, what + ' dbias')
  assert_equal(dWd, dW_ref if use_dW else w0, what + ' dW')
  assert_equal(am, dX_ref.abs().max().reshape(1), what + ' absmax')


def rowdot_outer_cases(act):
  """a block's 256 / (C / 4) lane groups own spans of 256 rows: one span + 1 and one block + 5 per width"""
  out = []
  n = 0
  for C in (4, 16, 64, 128, 256):
    block = (256 // (C // 4)) * SPAN
    for N in (1, 3, SPAN + 1, block + 5):
      out.append(dict(N=N, C=C, act=act, bias=n % 5 != 4, dW=n % 3 != 2))
      n += 1
  return out


# ---------------------------------------------------------------------------------------------------------------------
# weighted mean / variance over the views of a point (mlp_network.py:115-119, oracle fused_mean_variance)
# ---------------------------------------------------------------------------------------------------------------------
def meanvar_inputs(P, V, C, seed, zero_weight=True):
  """x, dvar integers in [-2, 2], w in {0, 1/2, 1} (a zero weight in every point with V > 1), dmean multiples of 1/2: the (x - mean)^2 dvar terms
  of dw stay below 24 bits"""
  g = gen(seed)
  x = torch.randint(-2, 3, (P, V, C), generator=g).double()
  w = torch.randint(0, 3, (P, V), generator=g).double() / 2
  if zero_weight and V > 1:
    w[:, V // 2] = 0.0
  return x, w, dyadic(g, P, C, den=2, lim=2), torch.randint(-2, 3, (P, C), generator=g).double(), dyadic(g, P, V, C, den=2, lim=2), dyadic(g, P, V, den=2, lim=2)


def meanvar_reference(x, w):
  mean, var = O.fused_mean_variance(x.unsqueeze(0), w.unsqueeze(0).unsqueeze(-1))
  return mean[0, :, 0], var[0, :, 0]


def check_meanvar(device, P, V, C, ld=None, accumulate=0, dw_accumulate=0, seed=0):
  """mean = sum_v x w, var = sum_v w (x - mean)^2 and their backward (dx (+)=, dw (+)=): the register forms (V <= 16; backward also C <= 128)
  and the general ones; everything equal to float64 autograd through the oracle's fused_mean_variance"""
  _p, stream_of, call = _api()
  ld = C if ld is None else ld
  what = f'meanvar P={P} V={V} C={C} ld={ld} acc={accumulate}/{dw_accumulate}'
  x, w, dmean, dvar, dx0, dw0 = meanvar_inputs(P, V, C, seed)
  xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
  mean, var = meanvar_reference(xg, wg)
  ((mean * dmean).sum() + (var * dvar).sum()).backward()
  _sum_exact(x * w[:, :, None], 1, what + ' mean')
  _sum_exact(w[:, :, None] * (x - mean.detach()[:, None]) ** 2, 1, what + ' var')
  dx_ref = _exact(xg.grad + (dx0 if accumulate else 0), what + ' dx')
  # dw[row] = sum_c [x dmean_t + (x - mean)^2 dvar], dmean_t = dmean - 2 dvar sum_v w (x - mean): the terms of the sum over the columns
  m = mean.detach()[:, None]
  dmt = (dmean - 2 * dvar * (w[:, :, None] * (x - m)).sum(1))[:, None]
  terms = torch.cat([x * dmt, (x - m) ** 2 * dvar[:, None], (dw0 * (1 if dw_accumulate else 0))[:, :, None]], 2)
  dw_ref = _sum_exact(terms, 2, what + ' dw')
  assert torch.equal(dw_ref, wg.grad + (dw0 if dw_accumulate else 0)), 'the stated terms of dw do not add up to autograd\'s gradient'
  N = P * V
  fx, _ = mat(x.reshape(N, C), ld, device, guard=16)  # (the register forms load 16 rows per point whatever V is: clamped, never past the point)
  w_d = dv(w.reshape(N), device)
  fst, vst = mat(torch.full((P, 2 * C), NAN), 2 * C + 4, device)  # [mean | var] side by side, as the callers keep them
  call('dyn_train_meanvar', _p(fx), ld, _p(w_d), P, V, C, _p(fst), _p(fst, C), 2 * C + 4, stream_of(fx))
  assert_equal(vst[:, :C], mean.detach(), what + ' mean')
  assert_equal(vst[:, C:2 * C], var.detach(), what + ' var')
  assert_pad(vst, 2 * C, what + ' mean / var')
  fg, _ = mat(torch.cat([dmean, dvar], 1), 2 * C + 4, device)
  fdx, vdx = mat((dx0 if accumulate else torch.full((P, V, C), NAN)).reshape(N, C), ld + 4, device)
  dw = dv((dw0 if dw_accumulate else torch.full((P, V), NAN)).reshape(N), device)
  # (dmean and dvar are two arrays of one leading dimension: the kernel takes `mean` with the same one)
  fmean, _ = mat(mean.detach(), 2 * C + 4, device)
  call('dyn_train_meanvar_bwd', _p(fx), ld, _p(w_d), P, V, C, _p(fmean), _p(fg), _p(fg, C), 2 * C + 4, _p(fdx), ld + 4, accumulate, _p(dw),
       dw_accumulate, stream_of(fx))
  assert_equal(vdx[:, :C], dx_ref.reshape(N, C), what + ' dx')
  assert_pad(vdx, C, what + ' dx')
  assert_equal(dw, dw_ref.reshape(N), what + ' dw')


def meanvar_cases():
  out = []
  n = 0
  for V, C, ld in ((1, 35, 36), (3, 70, 72), (8, 128, 128), (16, 35, 35), (17, 35, 36), (20, 70, 72), (8, 200, 200), (20, 200, 204), (16, 128, 132)):
    for P in (1, 3, 4, 5):
      out.append(dict(P=P, V=V, C=C, ld=ld, accumulate=n & 1, dw_accumulate=(n >> 1) & 1))
      n += 1
  # every pair of flags in the register and in the general form
  return out + [dict(P=5, V=V, C=70, ld=72, accumulate=a, dw_accumulate=b) for V in (8, 17) for a in (0, 1) for b in (0, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# pooling weights over the views (mlp_network.py:452-459, :470-471, :476; oracle static_net)
# ---------------------------------------------------------------------------------------------------------------------
def view_weights0_restatement(dot, mask, s):
  """anti-alias pooling weights.  dot, mask [P, V]; s a scalar (or None: weight = mask / (sum mask + 1e-8)); dtype follows the inputs"""
  if s is None:
    return mask / (torch.sum(mask, dim=1, keepdim=True) + 1e-8)
  e = torch.exp(torch.abs(s) * (dot - 1))
  weight = (e - torch.min(e, dim=1, keepdim=True)[0]) * mask
  return weight / (torch.sum(weight, dim=1, keepdim=True) + 1e-8)


def view_weights1_restatement(logit, mask):
  vis = torch.sigmoid(logit) * mask
  weight = vis / (torch.sum(vis, dim=1, keepdim=True) + 1e-8)
  return vis, weight, weight.mean(dim=1), torch.sum(mask, dim=1)


def view_weights_inputs(P, V, seed):
  g = gen(seed)
  dot = (1.0 - torch.rand(P, V, generator=g) * 0.3).double()  # cosines of the angle between query and source rays
  logit = torch.randn(P, V, generator=g).double() * 2
  mask = (torch.rand(P, V, generator=g) < 0.7).double()
  mask[P // 2] = 0.0  # a fully masked point
  if P > 1:
    mask[0] = 1.0
  return dot, logit, mask, torch.randn(P, V, generator=g).double(), torch.randn(P, V, generator=g).double(), torch.randn(P, generator=g).double()


def check_view_weights(device, P, V, mode, s=None, direct=True, seed=0):
  """mode 0: w (with |s|: e - min e; without: mask / count) and ds (accumulated by atomics; the sign of s by torch.abs's convention, 0 at s = 0).
  mode 1: vis, w, wmean, nvalid (equal) and dlogit from dw (+ dvis_direct, + dwmean).  `in` is column 3 of ray_diff (stride 4) in mode 0 and a
  column of a 2-wide matrix in mode 1, vis / dlogit / wmean are strided as the callers keep them."""
  _p, stream_of, call = _api()
  what = f'view_weights mode={mode} P={P} V={V} s={s} direct={direct}'
  dot, logit, mask, dw, dvis, dwm = view_weights_inputs(P, V, seed)
  N = P * V
  m_d, dw_d = dv(mask.reshape(N), device), dv(dw.reshape(N), device)
  w_out = torch.full((N,), NAN, device=device)
  if mode == 0:
    fin, _ = mat(dot.reshape(N, 1), 4, device, off=3)
    s_d = None if s is None else dv(torch.tensor([s]), device)
    call('dyn_train_view_weights', 0, _p(fin, 3) if s is not None else None, 4, _p(m_d), None if s is None else _p(s_d), P, V, _p(w_out), None, 0,
         None, 0, None, stream_of(m_d))
    ref, r32 = {}, {}
    for dt, o in ((torch.float64, ref), (torch.float32, r32)):
      # one s per row, so that the terms of the sum ds = sum_rows are visible (the minimum's share goes to the row that holds it)
      sv = None if s is None else torch.full((P, V), s, dtype=dt).requires_grad_(True)
      o['w'] = view_weights0_restatement(dot.to(dt), mask.to(dt), sv)
      if s is not None:
        (o['w'] * dw.to(dt)).sum().backward()
        o['terms'] = sv.grad
    assert_within(w_out, r32['w'].detach(), ref['w'].detach(), what + ' w')
    if s is not None:
      ds0 = 0.375
      ds = torch.full((1,), ds0, device=device)
      w_in = dv(ref['w'].detach().reshape(N), device)
      call('dyn_train_view_weights_bwd', 0, _p(fin, 3), 4, _p(m_d), _p(s_d), P, V, _p(w_in), _p(dw_d), None, 0, None, 0, None, 0, None, 0, _p(ds),
           stream_of(m_d))
      if s == 0.0:
        assert_equal(ds, torch.tensor([ds0]).double(), what + ' ds (torch.abs has gradient 0 at 0)')
      else:
        assert_within(ds - ds0, r32['terms'].sum().reshape(1), ref['terms'].sum().reshape(1), what + ' ds', magnitude=float(ref['terms'].abs().sum()) + ds0)
    return
  fin, _ = mat(logit.reshape(N, 1), 2, device)
  fvis, vvis = mat(torch.full((N, 1), NAN), 3, device)
  fwm, vwm = mat(torch.full((P, 1), NAN), 5, device)
  nvalid = torch.full((P,), NAN, device=device)
  call('dyn_train_view_weights', 1, _p(fin), 2, _p(m_d), None, P, V, _p(w_out), _p(fvis), 3, _p(fwm), 5, _p(nvalid), stream_of(m_d))
  ref, r32 = {}, {}
  for dt, o in ((torch.float64, ref), (torch.float32, r32)):
    lg = leaf(logit, dt)
    o['vis'], o['w'], o['wmean'], o['nvalid'] = view_weights1_restatement(lg, mask.to(dt))
    loss = (o['w'] * dw.to(dt)).sum()
    if direct:
      loss = loss + (o['vis'] * dvis.to(dt)).sum() + (o['wmean'] * dwm.to(dt)).sum()
    loss.backward()
    o['dlogit'] = lg.grad
  for k, got in (('vis', vvis[:, 0]), ('w', w_out), ('wmean', vwm[:, 0])):
    assert_within(got, r32[k].detach(), ref[k].detach(), f'{what} {k}')
  assert_equal(nvalid, ref['nvalid'], what + ' nvalid')
  assert_pad(vvis, 1, what + ' vis')
  assert_pad(vwm, 1, what + ' wmean')
  fdl, vdl = mat(torch.full((N, 1), NAN), 3, device)
  w_in, fvin = dv(ref['w'].detach().reshape(N), device), mat(ref['vis'].detach().reshape(N, 1), 3, device)[0]
  fdv, fdwm = mat(dvis.reshape(N, 1), 2, device)[0], mat(dwm[:, None], 5, device)[0]
  call('dyn_train_view_weights_bwd', 1, _p(fin), 2, _p(m_d), None, P, V, _p(w_in), _p(dw_d), _p(fdv) if direct else None, 2, _p(fvin), 3,
       _p(fdwm) if direct else None, 5, _p(fdl), 3, None, stream_of(m_d))
  assert_within(vdl[:, 0], r32['dlogit'], ref['dlogit'], what + ' dlogit')
  assert_pad(vdl, 1, what + ' dlogit')


def view_weights_cases():
  out = []
  n = 0
  for V in (1, 3, 8, 20):
    for P in (1, 255, 256, 257, 300):
      out.append(dict(P=P, V=V, mode=0, s=(0.75, -0.75, None, 0.0, 0.25)[n % 5]))
      out.append(dict(P=P, V=V, mode=1, direct=n % 2 == 0))
      n += 1
  return out + [dict(P=257, V=8, mode=0, s=s) for s in (0.75, -0.75, None, 0.0)]


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm over 128 columns of a + b (the attention block's residual, mlp_network.py:97; oracle ray_attention)
# ---------------------------------------------------------------------------------------------------------------------
def layernorm_restatement(y, gamma, beta):
  mean = y.mean(-1, keepdim=True)
  d = y - mean
  rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + 1e-6)
  xhat = d * rstd
  return xhat * gamma + beta, xhat, rstd[:, 0]


def layernorm_inputs(P, seed):
  g = gen(seed)
  a, b = torch.randn(P, 128, generator=g).double(), torch.randn(P, 128, generator=g).double()
  a[::3] += 40.0  # rows with a large common offset (the statistics are of deviations from the mean)
  a = a.float().double()
  return a, b, (1 + 0.3 * torch.randn(128, generator=g)).double(), torch.randn(128, generator=g).double(), torch.randn(P, 128, generator=g).double()


def check_layernorm(device, P, seed=0):
  """forward (out, xhat, rstd) and backward (din; dgamma / dbeta accumulated by atomics over 16 rows per wave, 64 per block).  The backward
  kernel takes the saved xhat / rstd: it gets the float64 ones (rounded), so its error is its own"""
  _p, stream_of, call = _api()
  what = f'layernorm P={P}'
  a, b, gamma, beta, dout = layernorm_inputs(P, seed)
  # the kernel adds a + b in fp32: both twins start from that sum, the rounding of which is the caller's input
  y = (a.float() + b.float())
  ref, r32 = {}, {}
  for dt, o in ((torch.float64, ref), (torch.float32, r32)):
    yy = leaf(y, dt)
    o['out'], o['xhat'], o['rstd'] = layernorm_restatement(yy, gamma.to(dt), beta.to(dt))
    o['out'].backward(dout.to(dt))
    o['din'] = yy.grad
    o['dg_terms'], o['db_terms'] = (dout.to(dt) * o['xhat']).detach(), dout.to(dt)
  out, xhat, rstd = (torch.full(s, NAN, device=device) for s in ((P, 128), (P, 128), (P,)))
  g_d, a_d = dv(gamma, device), dv(a, device)
  call('dyn_train_layernorm', _p(a_d), _p(dv(b, device)), _p(g_d), _p(dv(beta, device)), P, _p(out), _p(xhat), _p(rstd), stream_of(a_d))
  for k, got in (('out', out), ('xhat', xhat), ('rstd', rstd)):
    assert_within(got, r32[k].detach(), ref[k].detach(), f'{what} {k}')
  din = torch.full((P, 128), NAN, device=device)
  g0, b0 = torch.full((128,), 0.5), torch.full((128,), -0.25)
  dgamma, dbeta = dv(g0, device), dv(b0, device)
  call('dyn_train_layernorm_bwd', _p(dv(dout, device)), _p(dv(ref['xhat'].detach(), device)), _p(dv(ref['rstd'].detach(), device)), _p(g_d), P, _p(din),
       _p(dgamma), _p(dbeta), stream_of(a_d))
  assert_within(din, r32['din'], ref['din'], what + ' din')
  for k, got, base in (('dg_terms', dgamma, 0.5), ('db_terms', dbeta, -0.25)):
    mag = float(ref[k].abs().sum(0).max()) + abs(base)
    assert_within(got - base, r32[k].sum(0), ref[k].sum(0), f'{what} {k[:2]}', magnitude=mag)


LAYERNORM_P = (1, 15, 16, 17, 63, 64, 65, 130)


# ---------------------------------------------------------------------------------------------------------------------
# colour blending over the views + density fill (mlp_network.py:503-527; oracle static_net's tail)
# ---------------------------------------------------------------------------------------------------------------------
def blend_restatement(logit, mask, rgb_in, sigma, nvalid):
  x = logit.masked_fill(mask == 0, -1e9)
  blend = F.softmax(x, dim=1)
  rgb = torch.sum(rgb_in * blend[:, :, None], dim=1)
  return blend, torch.cat([rgb, sigma.masked_fill(nvalid < 1, -1e9)[:, None]], dim=-1)


def head_inputs(P, V, seed):
  g = gen(seed)
  mask = (torch.rand(P, V, generator=g) < 0.6).double()
  mask[0] = 0.0                      # a fully masked point (nvalid 0)
  if P > 2:
    mask[1] = 0.0
    mask[1, 0] = 1.0                 # nvalid 1
    mask[2, :2] = 1.0
    mask[2, 2:] = 0.0                # nvalid 2 (V >= 2)
  return mask, mask.sum(1)


def check_blend(device, P, V, seed=0):
  _p, stream_of, call = _api()
  what = f'blend P={P} V={V}'
  mask, nvalid = head_inputs(P, V, seed)
  g = gen(seed + 1)
  logit, feat = torch.randn(P, V, generator=g).double() * 2, torch.rand(P, V, 35, generator=g).double()
  sigma, draw = torch.randn(P, generator=g).double(), torch.randn(P, 4, generator=g).double()
  N = P * V
  ref, r32 = {}, {}
  for dt, o in ((torch.float64, ref), (torch.float32, r32)):
    lg, sg = leaf(logit, dt), leaf(sigma, dt)
    o['blend'], o['raw'] = blend_restatement(lg, mask.to(dt), feat[..., :3].to(dt), sg, nvalid.to(dt))
    (o['raw'] * draw.to(dt)).sum().backward()
    o['dlogit'], o['dsigma'] = lg.grad, sg.grad
  flg, _ = mat(logit.reshape(N, 1), 2, device)
  fsg, _ = mat(sigma[:, None], 3, device)
  m_d, f_d, nv_d = dv(mask.reshape(N), device), dv(feat.reshape(N, 35), device), dv(nvalid, device)
  blend, raw = torch.full((N,), NAN, device=device), torch.full((P, 4), NAN, device=device)
  call('dyn_train_blend', _p(flg), 2, _p(m_d), _p(f_d), _p(fsg), 3, _p(nv_d), P, V, _p(blend), _p(raw), stream_of(m_d))
  assert_within(blend, r32['blend'].detach(), ref['blend'].detach(), what + ' blend')
  assert_within(raw[:, :3], r32['raw'][:, :3].detach(), ref['raw'][:, :3].detach(), what + ' rgb')
  assert_equal(raw[:, 3], ref['raw'][:, 3].detach().float().double(), what + ' sigma (copied, or -1e9 where no view sees the point)')
  fdl, vdl = mat(torch.full((N, 1), NAN), 2, device)
  fds, vds = mat(torch.full((P, 1), NAN), 3, device)
  call('dyn_train_blend_bwd', _p(dv(draw, device)), _p(dv(ref['blend'].detach().reshape(N), device)), _p(m_d), _p(f_d), _p(nv_d), P, V, _p(fdl), 2,
       _p(fds), 3, stream_of(m_d))
  assert_within(vdl[:, 0], r32['dlogit'], ref['dlogit'], what + ' dlogit')
  assert_equal(vds[:, 0], ref['dsigma'].float().double(), what + ' dsigma')
  assert_pad(vdl, 1, what + ' dlogit')
  assert_pad(vds, 1, what + ' dsigma')


# colour / density head of the dynamic net (mlp_network.py:295-315; oracle dynamic_net's tail)
def dynamic_head_restatement(logit, sigma, nvalid, shift):
  sg = (sigma - shift).masked_fill(nvalid < 1, -1e9)
  rgb = torch.sigmoid(logit).masked_fill((nvalid == 0)[:, None].expand(-1, 3), 0)
  return torch.cat([rgb, sg[:, None]], dim=-1)


def check_dynamic_head(device, P, shift=5.0, seed=0):
  _p, stream_of, call = _api()
  what = f'dynamic_head P={P}'
  _, nvalid = head_inputs(P, 4, seed)
  g = gen(seed + 1)
  logit, sigma, draw = torch.randn(P, 3, generator=g).double() * 2, torch.randn(P, generator=g).double() * 3, torch.randn(P, 4, generator=g).double()
  ref, r32 = {}, {}
  for dt, o in ((torch.float64, ref), (torch.float32, r32)):
    lg, sg = leaf(logit, dt), leaf(sigma, dt)
    o['raw'] = dynamic_head_restatement(lg, sg, nvalid.to(dt), shift)
    (o['raw'] * draw.to(dt)).sum().backward()
    o['dlogit'], o['dsigma'] = lg.grad, sg.grad
  flg, _ = mat(logit, 4, device)
  nv_d = dv(nvalid, device)
  raw = torch.full((P, 4), NAN, device=device)
  call('dyn_train_dynamic_head', _p(flg), 4, _p(dv(sigma, device)), _p(nv_d), float(shift), P, _p(raw), stream_of(nv_d))
  assert_within(raw[:, :3], r32['raw'][:, :3].detach(), ref['raw'][:, :3].detach(), what + ' rgb')
  seen = nvalid >= 1
  assert_equal(raw[:, 3][~seen.to(raw.device)], torch.full((int((~seen).sum()),), -1e9).double(), what + ' sigma of unseen points')
  # sigma - shift is ONE fp32 subtraction: correctly rounded
  assert_equal(raw[:, 3][seen.to(raw.device)], (sigma.float() - shift)[seen].double(), what + ' sigma - shift')
  fdl, vdl = mat(torch.full((P, 3), NAN), 4, device)
  dsg = torch.full((P,), NAN, device=device)
  call('dyn_train_dynamic_head_bwd', _p(dv(draw, device)), _p(dv(ref['raw'].detach(), device)), _p(nv_d), P, _p(fdl), 4, _p(dsg), stream_of(nv_d))
  assert_within(vdl[:, :3], r32['dlogit'], ref['dlogit'], what + ' dlogit')
  assert_pad(vdl, 3, what + ' dlogit')
  assert_equal(dsg, ref['dsigma'].float().double(), what + ' dsigma')


HEAD_P = (1, 3, 255, 256, 257)


# ---------------------------------------------------------------------------------------------------------------------
# broadcast add, zeroing of a ray's last samples, f = [rgb_feat | src_feat * ref_feat]: exact
# ---------------------------------------------------------------------------------------------------------------------
def check_add_table(device, rows, C, period, seed=0):
  """y[row] = x[row] + tab[row % period] (period 1: one vector for every row; period S: the positional table of a ray)"""
  _p, stream_of, call = _api()
  what = f'add_table rows={rows} C={C} period={period}'
  g = gen(seed)
  x, tab = dyadic(g, rows, C), dyadic(g, period, C)
  ref = _exact(x + tab[torch.arange(rows) % period], what)
  fx, _ = mat(x, C, device)
  ft, _ = mat(tab, C + 1, device)
  fy, vy = mat(torch.full((rows, C), NAN), C + 1, device)
  call('dyn_train_add_table', _p(fx), C, _p(ft), C + 1, period, rows, C, _p(fy), C + 1, stream_of(fx))
  assert_equal(vy[:, :C], ref, what)
  assert_pad(vy, C, what)


def check_zero_tail(device, R, S, C, n_last, scale=0.5, seed=0):
  """x[r, s, :] = 0 for the last n_last samples of every ray, the rest scaled (render_ray.py:961, :1129)"""
  _p, stream_of, call = _api()
  what = f'zero_tail R={R} S={S} C={C} n_last={n_last}'
  x = dyadic(gen(seed), R, S, C)
  ref = _exact(x * scale, what)
  ref[:, S - n_last:] = 0.0
  x_d = dv(x, device)
  call('dyn_train_zero_tail', _p(x_d), R, S, C, n_last, float(scale), stream_of(x_d))
  assert_equal(x_d, ref, what)


def check_build_f(device, R, rows_per_ray, seed=0):
  """f = [rgb_feat (35) | src_feat * ref_feat[ray] (35) | 0 0] (mlp_network.py:450) and its backward: d src_feat = df[:, 35:70] ref_feat[ray],
  d ref_feat[ray] = sum over the ray's rows of df[:, 35:70] src_feat"""
  _p, stream_of, call = _api()
  what = f'build_f R={R} rows_per_ray={rows_per_ray}'
  N = R * rows_per_ray
  g = gen(seed)
  rgb, src, rf, df = dyadic(g, N, 35), dyadic(g, N, 35, lim=2), dyadic(g, R, 35, lim=2), dyadic(g, N, 70, lim=2)
  srcg, rfg = src.clone().requires_grad_(True), rf.clone().requires_grad_(True)
  f_ref = torch.cat([rgb, srcg * rfg.repeat_interleave(rows_per_ray, 0)], 1)
  (f_ref * df).sum().backward()
  _exact(f_ref.detach(), what)
  _sum_exact((df[:, 35:] * src).view(R, rows_per_ray, 35), 1, what + ' dref')
  fsrc, _ = mat(src, 36, device)
  frf, _ = mat(rf, 36, device)
  f = torch.full((N, 72), NAN, device=device)
  call('dyn_train_build_f', _p(dv(rgb, device)), _p(fsrc), 36, _p(frf), 36, N, rows_per_ray, _p(f), stream_of(f))
  assert_equal(f[:, :70], f_ref.detach(), what + ' f')
  assert_equal(f[:, 70:], torch.zeros(N, 2).double(), what + ' f zero columns')
  fdf, _ = mat(df, 72, device)
  fds, vds = mat(torch.full((N, 35), NAN), 36, device)
  fdr, vdr = mat(torch.full((R, 35), NAN), 36, device)
  call('dyn_train_build_f_bwd', _p(fdf), 72, _p(fsrc), 36, _p(frf), 36, R, rows_per_ray, _p(fds), 36, _p(fdr), 36, stream_of(f))
  assert_equal(vds[:, :35], _exact(srcg.grad, what), what + ' dsrc')
  assert_equal(vdr[:, :35], _exact(rfg.grad, what), what + ' dref')
  assert_pad(vds, 35, what + ' dsrc')
  assert_pad(vdr, 35, what + ' dref')


# ---------------------------------------------------------------------------------------------------------------------
# Fourier features (mlp_network.py:530-555; oracle periodic_embed) and Pluecker coordinates (render_ray.py:372-396)
# ---------------------------------------------------------------------------------------------------------------------
def _host_freqs(freqs):
  arr = (ctypes.c_float * 16)(*([float(f) for f in freqs] + [0.0] * (16 - len(freqs))))
  return arr, ctypes.cast(arr, ctypes.c_void_p)


def embed_restatement(x, freqs):
  """periodic_embed with the frequencies spelt out (octaves for the 5- and 4-octave embeds, linspace(1, 17, 16) for the motion MLP)"""
  out = [x]
  for fn in (torch.cos, torch.sin):
    for f in freqs:
      out.append(fn(f * x))
  return torch.cat(out, -1)


def check_embed(device, rows, D, freqs, accumulate=0, seed=0):
  """out = [x | cos(f x) ... | sin(f x) ...] and dx (+)= the gradient; x is the leading D columns of a wider matrix"""
  _p, stream_of, call = _api()
  nf = len(freqs)
  what = f'embed rows={rows} D={D} n_freqs={nf} acc={accumulate}'
  g = gen(seed)
  x, dout, dx0 = torch.randn(rows, D, generator=g).double(), torch.randn(rows, D * (1 + 2 * nf), generator=g).double(), torch.randn(rows, D, generator=g).double()
  f32 = [float(torch.tensor(f, dtype=torch.float32)) for f in freqs]  # the kernel receives fp32 frequencies: both twins use those
  ref, r32 = {}, {}
  for dt, o in ((torch.float64, ref), (torch.float32, r32)):
    xx = leaf(x.float(), dt)
    o['out'] = embed_restatement(xx, f32)
    o['out'].backward(dout.float().to(dt))
    o['dx'] = xx.grad + (dx0.float().to(dt) if accumulate else 0)
  W = D * (1 + 2 * nf)
  arr, fp = _host_freqs(freqs)
  fx, _ = mat(x, D + 1, device)
  fo, vo = mat(torch.full((rows, W), NAN), W + 3, device)
  call('dyn_train_embed', _p(fx), D + 1, rows, D, fp, nf, _p(fo), W + 3, stream_of(fx))
  assert_within(vo[:, :W], r32['out'].detach(), ref['out'].detach(), what + ' out')
  assert_pad(vo, W, what + ' out')
  fdo, _ = mat(dout, W + 3, device)
  fdx, vdx = mat(dx0 if accumulate else torch.full((rows, D), NAN), D + 2, device)
  call('dyn_train_embed_bwd', _p(fx), D + 1, rows, D, fp, nf, _p(fdo), W + 3, _p(fdx), D + 2, accumulate, stream_of(fx))
  # a sum of 2 n_freqs products of magnitude f |dout|: the magnitude of the cancelling sum is that of its terms
  mag = float((dout.abs()[:, :D] + sum(f * (dout.abs()[:, D + k * D:D + (k + 1) * D] + dout.abs()[:, D + (nf + k) * D:D + (nf + k + 1) * D])
                                       for k, f in enumerate(f32))).max())
  assert_within(vdx[:, :D], r32['dx'], ref['dx'], what + ' dx', magnitude=mag)
  assert_pad(vdx, D, what + ' dx')


OCTAVES5 = (1.0, 2.0, 4.0, 8.0, 16.0)
MOTION_FREQS = tuple(float(f) for f in torch.linspace(1, 17, 16))  # periodic_embed(x, 16, 16, linspace=True) of the motion MLP


def embed_cases():
  return [dict(rows=r, D=D, freqs=f, accumulate=a) for r, D, f, a in ((1, 3, OCTAVES5, 0), (85, 3, OCTAVES5, 1), (86, 3, OCTAVES5, 0), (257, 4, MOTION_FREQS, 0),
                                                                         (64, 4, MOTION_FREQS, 1), (65, 1, (1.0,), 0), (7, 2, (), 1))]


def dynamic_embed_restatement(pts, ray_d):
  """pts_pe = PE_5(pts) (33), dir_pe = PE_4(F.normalize(ray_d)) (27)"""
  return O.periodic_embed(pts, 5, 5, False), O.periodic_embed(F.normalize(ray_d, dim=-1), 4, 4, False)


def _rays(R, g):
  d = torch.randn(R, 3, generator=g).double()
  d[-1] = 0.0  # a zero-length direction: F.normalize's clamp (1e-12) leaves zeros
  return torch.randn(R, 3, generator=g).double(), d


def check_dynamic_embed(device, P, R, seed=0):
  _p, stream_of, call = _api()
  what = f'dynamic_embed P={P} R={R}'
  g = gen(seed)
  pts = torch.randn(P, 3, generator=g).double() * 2
  _, ray_d = _rays(R, g)
  ref = dynamic_embed_restatement(pts.float().double(), ray_d.float().double())
  r32 = dynamic_embed_restatement(pts.float(), ray_d.float())
  ppe, dpe = torch.full((P, 36), NAN, device=device), torch.full((R, 28), NAN, device=device)
  call('dyn_train_dynamic_embed', _p(dv(pts, device)), _p(dv(ray_d, device)), P, R, _p(ppe), _p(dpe), stream_of(ppe))
  assert_within(ppe[:, :33], r32[0], ref[0], what + ' pts_pe')
  assert_within(dpe[:, :27], r32[1], ref[1], what + ' dir_pe')
  assert_equal(ppe[:, 33:], torch.zeros(P, 3).double(), what + ' pts_pe zero columns')
  assert_equal(dpe[:, 27:], torch.zeros(R, 1).double(), what + ' dir_pe zero column')


def static_embed_restatement(pts, ray_o, ray_d, centers, ray_diff, feat, mask, mask_rgb):
  """a0 = [PE(pts) | PE(src Pluecker) | ray_diff], ref_pe = PE(ref Pluecker), mask_eff (oracle static_net's head; torch.cross without dim as the
  reference calls it).  pts [R, S, 3], centers [V, 3], ray_diff [R, S, V, 4], feat [R, S, V, 35], mask [R, S, V]"""
  R, S, V = mask.shape
  cams = torch.zeros(1, V, 34, dtype=pts.dtype)
  c2w = torch.eye(4, dtype=pts.dtype).repeat(V, 1, 1)
  c2w[:, :3, 3] = centers
  cams[0, :, -16:] = c2w.reshape(V, 16)
  ref_pe = O.periodic_embed(O.ref_plucker(ray_o, ray_d), 5, 5, False)
  src_pe = O.periodic_embed(O.src_plucker(pts, cams), 5, 5, False)
  pts_pe = O.periodic_embed(pts, 5, 5, False)
  a0 = torch.cat([pts_pe.unsqueeze(2).expand(-1, -1, V, -1), src_pe, ray_diff], dim=-1)
  if mask_rgb:
    mask = mask * (torch.sum(feat[..., :3], dim=-1) > 1e-3).to(pts.dtype)
  return a0.reshape(R * S * V, 103), ref_pe, mask.reshape(-1)


def check_static_embed(device, R, S, V, mask_rgb, seed=0):
  """V = 3 follows the reference's torch.cross over the view axis (check_cross_axis pins the oracle's reading of it)"""
  _p, stream_of, call = _api()
  what = f'static_embed R={R} S={S} V={V} mask_rgb={mask_rgb}'
  g = gen(seed)
  N = R * S * V
  pts, centers = torch.randn(R, S, 3, generator=g).double() * 2, torch.randn(V, 3, generator=g).double()
  ray_o, ray_d = _rays(R, g)
  pts[0, 0] = centers[V - 1]  # a point on a camera centre: a zero-length source ray
  rd, feat = torch.randn(R, S, V, 4, generator=g).double(), torch.rand(R, S, V, 35, generator=g).double()
  feat[:, :, ::2, :3] *= 1e-4  # dark source pixels: dropped by mask_rgb
  feat = feat.float().double()
  mask = (torch.rand(R, S, V, generator=g) < 0.7).double()
  f = lambda t: t.float().double()
  ref = static_embed_restatement(f(pts), f(ray_o), f(ray_d), f(centers), f(rd), f(feat), mask, mask_rgb)
  r32 = static_embed_restatement(pts.float(), ray_o.float(), ray_d.float(), centers.float(), rd.float(), feat.float(), mask.float(), mask_rgb)
  fc, _ = mat(centers, 16, device, off=12)  # the translation column of row-major [V, 4, 4]-like records, as the callers pass it
  a0, refpe, meff = torch.full((N, 104), NAN, device=device), torch.full((R, 68), NAN, device=device), torch.full((N,), NAN, device=device)
  call('dyn_train_static_embed', _p(dv(pts.reshape(-1, 3), device)), _p(dv(ray_o, device)), _p(dv(ray_d, device)), _p(fc, 12), 16,
       _p(dv(rd.reshape(N, 4), device)), _p(dv(feat.reshape(N, 35), device)), _p(dv(mask.reshape(N), device)), R, S, V, int(mask_rgb), _p(a0), _p(refpe),
       _p(meff), stream_of(a0))
  assert_within(a0[:, :99], r32[0][:, :99], ref[0][:, :99], what + ' a0 Fourier features')
  assert_equal(a0[:, 99:103], ref[0][:, 99:], what + ' a0 ray_diff')
  assert_equal(a0[:, 103:], torch.zeros(N, 1).double(), what + ' a0 zero column')
  assert_within(refpe[:, :66], r32[1], ref[1], what + ' ref_pe')
  assert_equal(refpe[:, 66:], torch.zeros(R, 2).double(), what + ' ref_pe zero columns')
  # the dark pixels are 1e-4 * U(0, 1) * 3 < 1e-3 and the bright ones ~ 1.5: no sum is near the threshold
  assert_equal(meff, ref[2], what + ' mask_eff')


def static_embed_cases():
  return [dict(R=2, S=5, V=3, mask_rgb=True), dict(R=5, S=7, V=8, mask_rgb=False), dict(R=4, S=9, V=8, mask_rgb=True), dict(R=2, S=4, V=3, mask_rgb=False),
          dict(R=1, S=1, V=1, mask_rgb=False)]


# ---------------------------------------------------------------------------------------------------------------------
# argument errors: rejected before any launch
# ---------------------------------------------------------------------------------------------------------------------
def check_argument_errors(device):
  """each message names its entry point"""
  import pytest
  _p, stream_of, call = _api()
  z = torch.zeros(64 * 264, device=device)
  st = stream_of(z)
  p = _p(z)
  with pytest.raises(RuntimeError, match='dyn_train_act_bwd'):
    call('dyn_train_act_bwd', p, p, 10, 16, 16, 16, 1, None, 3, p, 16, None, st)
  with pytest.raises(RuntimeError, match='dyn_train_rowdot'):
    call('dyn_train_rowdot', p, 12, p, None, 4, 12, p, 1, st)
  with pytest.raises(RuntimeError, match='dyn_train_outer_act_bwd'):
    call('dyn_train_outer_act_bwd', p, 1, p, p, 12, 4, 12, 1, p, 12, None, None, None, st)
  with pytest.raises(RuntimeError, match='dyn_train_outer_act_bwd'):
    call('dyn_train_outer_act_bwd', p, 1, p, None, 16, 4, 16, 0, p, 16, None, None, p, st)
  with pytest.raises(RuntimeError, match='dyn_train_vis_split_act_bwd'):
    call('dyn_train_vis_split_act_bwd', p, 128, p, p, 130, p, 4, p, 132, None, None, None, 0, None, 0, None, st)
  with pytest.raises(RuntimeError, match='dyn_train_meanvar_bwd'):
    call('dyn_train_meanvar_bwd', p, 257, p, 1, 2, 257, p, p, p, 257, p, 257, 0, p, 0, st)


# ---------------------------------------------------------------------------------------------------------------------
# the table the device and the emulator suites both walk: group -> (check, cases)
# ---------------------------------------------------------------------------------------------------------------------
def _kw(rows, cols, act, kw):
  return dict(rows=rows, cols=cols, act=act, **kw)


GROUPS = {
    'act_bwd': (check_act_bwd, [_kw(*c) for c in act_bwd_cases()]),
    'absmax': (check_absmax, absmax_cases()),
    'colsum_reduce': (check_colsum_reduce, colsum_reduce_cases()),
    'rowscale': (check_rowscale, rowscale_cases()),
    'rowscale_act_bwd-act0': (check_rowscale_act_bwd, rowscale_act_bwd_cases(0)),
    'rowscale_act_bwd-act1': (check_rowscale_act_bwd, rowscale_act_bwd_cases(1)),
    'rowscale_act_bwd-act2': (check_rowscale_act_bwd, rowscale_act_bwd_cases(2)),
    'vis_split': (check_vis_split, [dict(N=N, ray_diff=bool(i & 1)) for i, N in enumerate((1, 7, 8, 9, 261))]),
    'vis_split_act_bwd-plain': (check_vis_split_act_bwd, vis_split_act_bwd_cases(False)),
    'vis_split_act_bwd-fused': (check_vis_split_act_bwd, vis_split_act_bwd_cases(True)),
    'rowdot_outer-act0': (check_rowdot_outer, rowdot_outer_cases(0)),
    'rowdot_outer-act1': (check_rowdot_outer, rowdot_outer_cases(1)),
    'rowdot_outer-act2': (check_rowdot_outer, rowdot_outer_cases(2)),
    'meanvar': (check_meanvar, meanvar_cases()),
    'view_weights': (check_view_weights, view_weights_cases()),
    'layernorm': (check_layernorm, [dict(P=P) for P in LAYERNORM_P]),
    'blend': (check_blend, [dict(P=P, V=V) for P in HEAD_P for V in (3, 8)]),
    'dynamic_head': (check_dynamic_head, [dict(P=P) for P in HEAD_P]),
    'add_table': (check_add_table, [dict(rows=r, C=C, period=p) for C in (35, 128) for r, p in ((1, 1), (67, 1), (64, 16), (300, 20))]),
    'zero_tail': (check_zero_tail, [dict(R=5, S=16, C=18, n_last=n) for n in (0, 1, 16)] + [dict(R=1, S=1, C=1, n_last=1), dict(R=3, S=37, C=6, n_last=4)]),
    'build_f': (check_build_f, [dict(R=1, rows_per_ray=1), dict(R=3, rows_per_ray=6), dict(R=2, rows_per_ray=7 * 8), dict(R=5, rows_per_ray=64 * 8 + 3)]),
    'embed': (check_embed, embed_cases()),
    'dynamic_embed': (check_dynamic_embed, [dict(P=1, R=1), dict(P=255, R=5), dict(P=257, R=257), dict(P=300, R=2)]),
    'static_embed': (check_static_embed, static_embed_cases()),
}


def run_group(device, name):
  fn, cases = GROUPS[name]
  for i, kw in enumerate(cases):
    fn(device, seed=17 * i + 1, **kw) if 'seed' not in kw else fn(device, **kw)
