"""Support for the tests of the extended optimizer step (dynibar_amd/optim.py, csrc/dyn_optim.h: k_adamx_step, k_adamx_step_guarded,
k_adam_advance -- weight decay in both forms, amsgrad, maximize, device-resident step counts): the numpy restatement of the contract of
include/dynibar_hip.h, the double arithmetic of the device's bias corrections included, a harness that mirrors an optimizer's tensors, and
the checks the emulator and the device tests share.  Test infrastructure: nothing in dynibar_amd imports this.

The kernels are compared with the restatement exactly (torch.equal; NaNs by position).  Against torch the check is closeness: over five steps
on parameters and gradients of order 1, d = max |torch fp32 - torch float64| per option set is torch's own rounding noise, and ours must stay
within 2 d of torch's float64 -- both are fp32 sequences of the same length with different roundings."""
import copy

import numpy as np
import torch

import optim_cases as oc
import optim_guard_cases as gc

F = np.float32
D = np.float64
SHAPES = [(), 1, 3, 4095, 4096, 4097, 8193]  # a 0-d tensor; below, at and above one chunk of 4096; two chunks and one element


# ---- the contract --------------------------------------------------------------------------------------------------------------------
def pow_scalars(lr, beta1, beta2, pw):
  """the device's scalars of the step after the t steps whose beta1^t, beta2^t are pw: double, every operation rounded once, then fp32 once
  -> (a, s2, the advanced pw)"""
  b1, b2 = D(pw[0]) * D(beta1), D(pw[1]) * D(beta2)
  with np.errstate(all='ignore'):
    a, s2 = F(-D(lr) / (D(1.0) - b1)), F(np.sqrt(D(1.0) - b2))
  return a, s2, np.array([b1, b2], D)


def decay_factor(lr, lam):
  """the decoupled factor: formed in double, rounded to fp32 once"""
  return F(1 - lr * lam)


def restate(p, g, m, v, vmax, a, s2, beta1, beta2, eps, coef=None, wd=0.0, decay=1.0, maximize=False):
  """one extended step on fp32 arrays -> (p, m, v, vmax); vmax None: no amsgrad.  coef None: the unguarded form"""
  assert p.dtype == g.dtype == m.dtype == v.dtype == np.float32 and (vmax is None or vmax.dtype == np.float32)
  c1, c2, b2, e = F(1 - beta1), F(1 - beta2), F(beta2), F(eps)
  a, s2 = F(a), F(s2)
  with np.errstate(all='ignore'):
    if maximize:
      g = -g
    if coef is not None:
      g = g * F(coef)
    if wd != 0:
      g = g + F(wd) * p
    p1 = p * F(decay)
    m = m + c1 * (g - m)
    v = v * b2 + (c2 * g) * g
    d = v
    if vmax is not None:
      vmax = np.where(v > vmax, v, vmax)  # a NaN v compares false: vmax stays
      d = vmax
    denom = np.sqrt(d) / s2 + e
    p = p1 + (a * m) / denom
  assert p.dtype == m.dtype == v.dtype == np.float32 and (vmax is None or vmax.dtype == np.float32)
  return p, m, v, vmax


# ---- the harness -----------------------------------------------------------------------------------------------------------------------
class Tensors(oc.Tensors):
  """oc.Tensors with the options of the extended step per group: the mirror also holds vmax (amsgrad) and pw = [beta1^t, beta2^t]
  (capturable), and a tensor that is a view starts from a loaded state with them."""

  def __init__(self, dev, groups, seed=0, offsets=None, extended_kernel=False):
    from dynibar_amd import optim
    basic = ('lr', 'betas', 'eps')  # (oc.Tensors builds an optim.Adam, which refuses the options: the same tensors and loaded state go to an AdamX)
    super().__init__(dev, [({k: v for k, v in o.items() if k in basic}, shapes) for o, shapes in groups], seed=seed, offsets=offsets)
    plain = self.opt
    self.opt = optim.AdamX([dict(params=g['params'], **o) for g, (o, _) in zip(plain.param_groups, groups)])
    for param, st in plain.state.items():
      self.opt.state[param] = st
    self.opt.extended_kernel = extended_kernel
    self.vmax, self.pw, self.xflats = [None] * len(self), [None] * len(self), {}
    for i, param in enumerate(self.params):
      grp = self.opt.param_groups[self.group_of[i]]
      n = self.p[i].size
      if grp['amsgrad']:
        self.vmax[i] = np.zeros(n, F)
      if grp['capturable']:
        self.pw[i] = np.ones(2, D)
      if i not in self.views:
        continue
      st = self.opt.state[param]
      if grp['amsgrad']:  # about half of the elements start above v, half below
        x0 = (self.v[i] * (0.5 + self.rng.random(n))).astype(F)
        flat = torch.full((n + oc.PAD,), oc.SENTINEL, dtype=torch.float32, device=dev)
        off = oc.LEAD + offsets[i][0]
        flat[off:off + n].copy_(torch.from_numpy(x0))
        self.xflats[i] = (flat, off)
        st['max_exp_avg_sq'] = flat[off:off + n].view(self.shapes[i])
        self.vmax[i] = x0
      if grp['capturable']:
        b1, b2 = grp['betas']
        self.pw[i] = np.array([b1 ** self.t[i], b2 ** self.t[i]], D)
        st['step'] = torch.tensor(float(self.t[i]), dtype=torch.float32, device=dev)
        st['beta_pow'] = torch.from_numpy(self.pw[i].copy()).to(dev)

  def step(self, grads, max_grad_norm=None, skip_nonfinite=False, zero_grads=False):
    from dynibar_amd import optim
    coef, held = None, False
    if max_grad_norm is not None or skip_nonfinite:
      table = [np.zeros(p.size, F) if g is None else g for g, p in zip(grads, self.p)]
      _, st = gc.restate_norm(table, optim.CHUNK, max_grad_norm)
      coef, held = st['coef'], bool(skip_nonfinite) and not st['finite']
    self.set_grads(grads)
    self.opt.step(zero_grads=zero_grads, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
    for i, g in enumerate(grads):
      if g is None:
        continue
      grp = self.opt.param_groups[self.group_of[i]]
      lr, (b1, b2) = grp['lr'], grp['betas']
      if self.pw[i] is not None:  # the count is the device's: a held step does not advance it
        if held:
          continue
        a, s2, self.pw[i] = pow_scalars(lr, b1, b2, self.pw[i])
        self.t[i] += 1
      else:                       # the count is the host's: it advances whatever the device did
        self.t[i] += 1
        if held:
          continue
        a, s2 = oc.scalars(lr, b1, b2, self.t[i])
      lam, dec = grp['weight_decay'], grp.get('decoupled_weight_decay', False)
      self.p[i], self.m[i], self.v[i], self.vmax[i] = restate(
          self.p[i], g, self.m[i], self.v[i], self.vmax[i], a, s2, b1, b2, grp['eps'], coef=coef, wd=0.0 if dec else lam,
          decay=decay_factor(lr, lam) if dec and lam != 0 else 1.0, maximize=grp['maximize'])
    return held

  def check(self):
    for i, param in enumerate(self.params):
      what = f'tensor {i} {self.shapes[i]} of group {self.group_of[i]}'
      oc.same(self.p[i], param, f'p of {what}')
      st = self.opt.state.get(param)
      if self.t[i] == 0 and i not in self.views:
        assert not st, f'{what} never had a gradient but has state {list(st)}'
        continue
      step = st['step']
      assert step.dtype == torch.float32 and step.dim() == 0
      assert step.device == (param.device if self.pw[i] is not None else torch.device('cpu')), f'{what}: step on {step.device}'
      assert float(step) == self.t[i], f'{what}: step {float(step)} != {self.t[i]}'
      oc.same(self.m[i], st['exp_avg'], f'm of {what}')
      oc.same(self.v[i], st['exp_avg_sq'], f'v of {what}')
      assert ('max_exp_avg_sq' in st) == (self.vmax[i] is not None) and ('beta_pow' in st) == (self.pw[i] is not None), (what, list(st))
      if self.vmax[i] is not None:
        assert st['max_exp_avg_sq'].shape == param.shape and st['max_exp_avg_sq'].device == param.device
        oc.same(self.vmax[i], st['max_exp_avg_sq'], f'vmax of {what}')
      if self.pw[i] is not None:
        pw = st['beta_pow']
        assert pw.dtype == torch.float64 and pw.shape == (2,) and pw.device == param.device
        gc.same64(self.pw[i], pw, f'beta_pow of {what}')
    for i, flats in self.flats.items():
      n = self.p[i].size
      for flat, view, name in list(zip(flats, self.views[i], 'pgmv')) + ([(self.xflats[i][0], None, 'vmax')] if i in self.xflats else []):
        off = self.xflats[i][1] if view is None else view.storage_offset()
        outside = torch.cat([flat[:off], flat[off + n:]]).cpu()
        assert outside.numel() == oc.PAD and torch.equal(outside, torch.full((oc.PAD,), oc.SENTINEL)), f'tensor {i}: {name} was written outside its view'

  def snapshot(self):
    """every bit of the optimizer's tensors, for comparisons between runs"""
    out = []
    for param in self.params:
      st = self.opt.state.get(param, {})
      out.append({'p': param.detach().cpu().clone(), **{k: v.detach().cpu().clone() for k, v in st.items()}})
    return out


def same_snapshots(a, b, what):
  assert len(a) == len(b)
  for i, (x, y) in enumerate(zip(a, b)):
    assert x.keys() == y.keys(), (what, i, list(x), list(y))
    for k in x:
      assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), f'{what}: {k} of tensor {i} differs'


def mixed_groups(capturable):
  """a plain group, a coupled-decay group, a decoupled amsgrad group and a maximize group, each with SHAPES twice (the second time as views one
  float off 16 bytes) -> (groups, offsets)"""
  cap = dict(capturable=True) if capturable else {}
  opts = [dict(lr=4e-4), dict(lr=1e-3, weight_decay=0.1), dict(lr=5e-4, betas=(0.8, 0.99), weight_decay=0.05, decoupled_weight_decay=True, amsgrad=True),
          dict(lr=2e-4, maximize=True, eps=1e-6)]
  groups = [(dict(o, **cap), SHAPES + SHAPES) for o in opts]
  offsets = {gi * 2 * len(SHAPES) + len(SHAPES) + k: (1, 1, 1, 1) for gi in range(len(opts)) for k in range(len(SHAPES))}
  return groups, offsets


def _guard_args(T, grads, guarded, s):
  if not guarded:
    return {}
  norm = float(gc.restate_norm([np.zeros(p.size, F) if g is None else g for g, p in zip(grads, T.p)], 4096)[1]['norm'])
  return dict(max_grad_norm=(0.5 if s % 2 == 0 else 4.0) * norm, skip_nonfinite=True)


# ---- the shared checks ---------------------------------------------------------------------------------------------------------------
BITWISE_CASES = [(guarded, zero_grads, capturable) for guarded in (False, True) for zero_grads in (False, True) for capturable in (False, True)]


def check_bitwise(dev, guarded, zero_grads, capturable):
  """the four groups in one launch, every shape aligned and as a view, tensor 3 without a gradient at the second step: p, m, v, vmax, step and
  beta_pow against the restatement after 1 and after 5 steps"""
  groups, offsets = mixed_groups(capturable)
  T = Tensors(dev, groups, seed=40 + 4 * guarded + 2 * zero_grads + capturable, offsets=offsets)
  assert len(T) == 56
  for s in range(5):
    grads = T.gradients()
    if s == 1:
      grads[3] = None
    held = T.step(grads, zero_grads=zero_grads, **_guard_args(T, grads, guarded, s))
    assert not held and T.opt._tables['extended']
    if s in (0, 4):
      T.check()
    if zero_grads:
      assert all(x.grad is None or not bool(x.grad.any()) for x in T.params)
  assert T.t[3] == 4 and T.t[2] == 5 and T.t[len(SHAPES)] == 7  # (a view starts from a loaded t = 2)


def check_single_float_path(dev, shape):
  """one tensor alone, aligned and one float off, with every option at once (AdamW + amsgrad + maximize + capturable), guarded"""
  opts = dict(lr=1e-3, weight_decay=0.1, decoupled_weight_decay=True, amsgrad=True, maximize=True, capturable=True)
  T = Tensors(dev, [(opts, [shape, shape])], seed=60 + oc.numel(shape), offsets={1: (1, 1, 1, 1)})
  for s in range(2):
    grads = T.gradients()
    T.step(grads, zero_grads=s == 1, **_guard_args(T, grads, True, s))
  T.check()


def check_old_path_unchanged(dev, guarded):
  """no option set: the extended kernels leave the bits of the plain entry points on the same inputs"""
  groups = [(dict(lr=4e-4), SHAPES + SHAPES), (dict(lr=1e-3, betas=(0.85, 0.995), eps=1e-6), SHAPES)]
  offsets = {len(SHAPES) + k: (1, 1, 1, 1) for k in range(len(SHAPES))}
  A, B = (Tensors(dev, groups, seed=70 + guarded, offsets=offsets, extended_kernel=x) for x in (False, True))
  for s in range(3):
    grads = A.gradients()
    B.gradients()
    for T in (A, B):
      T.step([None if g is None else g.copy() for g in grads], zero_grads=s == 2, **_guard_args(T, grads, guarded, s))
  assert not A.opt._tables['extended'] and B.opt._tables['extended']
  A.check()
  same_snapshots(A.snapshot(), B.snapshot(), 'plain against extended entry points')


def _skip_run(dev, capturable, steps):
  shapes = [(), 3, 4097, (), 4097]  # per group: three tensors aligned, two as views (a held step must leave every path's tensors alone)
  groups = [(o, shapes) for o, _ in mixed_groups(capturable)[0]]
  offsets = {gi * len(shapes) + 3 + k: (1, 1, 1, 1) for gi in range(4) for k in range(2)}
  T = Tensors(dev, groups, seed=80, offsets=offsets)
  finite = [T.gradients() for _ in range(4)]
  bad = [g.copy() for g in T.gradients()]
  bad[2][4096] = np.inf  # one element, in the second chunk of a 4097-element tensor
  order = dict(all=[finite[0], finite[1], bad, finite[2], finite[3]], finite=finite)[steps]
  held = [T.step([g.copy() for g in grads], max_grad_norm=1.0, skip_nonfinite=True) for grads in order]
  return T, held


def check_exact_skip(dev):
  """steps 1-2 finite, step 3 with one Inf element, steps 4-5 finite.  capturable: every bit equals the run of the four finite steps alone and
  step == 4.  Not capturable: the host's count is 5, as documented."""
  T, held = _skip_run(dev, True, 'all')
  assert held == [False, False, True, False, False]
  T.check()
  R, _ = _skip_run(dev, True, 'finite')
  same_snapshots(R.snapshot(), T.snapshot(), 'five steps with a held one against the four finite steps')
  base = [2 if i in T.views else 0 for i in range(len(T))]
  assert all(float(T.opt.state[x]['step']) == 4 + b for x, b in zip(T.params, base))
  assert int(T.opt.grad_stats.nonfinite) == 1 and int(T.opt.grad_stats.calls) == 5
  H, held = _skip_run(dev, False, 'all')
  assert held == [False, False, True, False, False]
  H.check()
  assert all(float(H.opt.state[x]['step']) == 5 + b and H.opt.state[x]['step'].device.type == 'cpu' for x, b in zip(H.params, base))


# ---- against torch -------------------------------------------------------------------------------------------------------------------
N_TORCH, LR_TORCH, STEPS = 4097, 1e-2, 5
OPTION_SETS = {
    'coupled': ('Adam', dict(weight_decay=0.1)),  # (torch's class name; ours is AdamX for torch's Adam, AdamW for its AdamW)
    'adamw': ('AdamW', dict(weight_decay=0.1)),
    'amsgrad': ('Adam', dict(amsgrad=True)),
    'maximize': ('Adam', dict(maximize=True)),
    'adamw_amsgrad_maximize': ('AdamW', dict(weight_decay=0.1, amsgrad=True, maximize=True)),
}
_TORCH = {}


def torch_data(name):
  rng = np.random.default_rng([sorted(OPTION_SETS).index(name), 5])
  return rng.standard_normal(N_TORCH).astype(F), [rng.standard_normal(N_TORCH).astype(F) for _ in range(STEPS + 1)]


def torch_reference(name):
  """torch.optim.Adam / AdamW on the CPU in float64 and in float32 over the five steps, computed once -> dict(p64, p32, d, opt32, q32): d is
  max |p32 - p64| after the five steps, opt32 / q32 the fp32 optimizer and its parameter (for the exchange of state_dicts)"""
  if name not in _TORCH:
    cls, kw = OPTION_SETS[name]
    p0, grads = torch_data(name)
    out = {}
    for dtype in (torch.float64, torch.float32):
      q = torch.nn.Parameter(torch.from_numpy(p0).to(dtype))
      opt = getattr(torch.optim, cls)([q], lr=LR_TORCH, **kw)
      for g in grads[:STEPS]:
        q.grad = torch.from_numpy(g).to(dtype)
        opt.step()
      out[dtype] = (q, opt)
    p64, p32 = out[torch.float64][0].detach().numpy().copy(), out[torch.float32][0].detach().numpy().copy()
    _TORCH[name] = dict(p64=p64, p32=p32, d=float(np.abs(p32.astype(D) - p64).max()), opt32=out[torch.float32][1], q32=out[torch.float32][0])
  return _TORCH[name]


def ours_class(torch_name):
  from dynibar_amd import optim
  return dict(Adam=optim.AdamX, AdamW=optim.AdamW)[torch_name]


def ours_for(dev, name, capturable=False):
  from dynibar_amd import optim
  cls, kw = OPTION_SETS[name]
  p0, grads = torch_data(name)
  q = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dev))
  return q, ours_class(cls)([q], lr=LR_TORCH, capturable=capturable, **kw), grads


def _step(q, opt, g, dev):
  q.grad = torch.from_numpy(g.copy()).to(dev)
  opt.step()


def check_against_torch(dev, name, capturable=False):
  ref = torch_reference(name)
  q, opt, grads = ours_for(dev, name, capturable)
  for g in grads[:STEPS]:
    _step(q, opt, g, dev)
  ours = float(np.abs(q.detach().cpu().numpy().astype(D) - ref['p64']).max())
  print(f'  {name}{" capturable" if capturable else ""}: d = max|torch32 - torch64| = {ref["d"]:.3e}   max|ours - torch64| = {ours:.3e}   ratio {ours / ref["d"]:.3f}')
  assert ref['d'] > 0 and ours <= 2 * ref['d'], (name, ours, ref['d'])
  return q, opt, grads


def check_interop(dev, name):
  """our state_dict into torch's optimizer of the same options and back; one further step from either side within 2 d"""
  cls, kw = OPTION_SETS[name]
  ref = torch_reference(name)
  q, opt, grads = check_against_torch(dev, name)
  # ours -> torch: a host copy of our parameter, torch's optimizer with our state, one further step on both sides
  theirs_q = torch.nn.Parameter(q.detach().cpu().clone())
  theirs = getattr(torch.optim, cls)([theirs_q], lr=LR_TORCH, **kw)
  theirs.load_state_dict(copy.deepcopy(opt.state_dict()))
  st = theirs.state[theirs_q]
  assert float(st['step']) == STEPS and torch.equal(st['exp_avg'], opt.state[q]['exp_avg'].cpu())
  assert ('max_exp_avg_sq' in st) == bool(kw.get('amsgrad'))
  theirs_q.grad = torch.from_numpy(grads[STEPS].copy())
  theirs.step()
  _step(q, opt, grads[STEPS], dev)
  dist = float((q.detach().cpu().double() - theirs_q.detach().double()).abs().max())
  print(f'  {name}: ours -> torch, one further step on both sides: distance {dist:.3e} (2 d = {2 * ref["d"]:.3e})')
  assert dist <= 2 * ref['d']
  # torch -> ours: the fp32 reference run's state into a fresh optimizer of ours, one further step on both sides
  back_q, back, _ = ours_for(dev, name)
  with torch.no_grad():
    back_q.copy_(ref['q32'].detach())
  theirs2 = copy.deepcopy(ref['opt32'])
  q2 = theirs2.param_groups[0]['params'][0]
  back.load_state_dict(copy.deepcopy(theirs2.state_dict()))
  assert back.state[back_q]['exp_avg'].device == back_q.device and float(back.state[back_q]['step']) == STEPS
  q2.grad = torch.from_numpy(grads[STEPS].copy())
  theirs2.step()
  _step(back_q, back, grads[STEPS], dev)
  dist = float((back_q.detach().cpu().double() - q2.detach().double()).abs().max())
  print(f'  {name}: torch -> ours, one further step on both sides: distance {dist:.3e} (2 d = {2 * ref["d"]:.3e})')
  assert dist <= 2 * ref['d']


def check_capturable_state(dev):
  """beta_pow through state_dict / load_state_dict bit for bit (torch's loader would round it to fp32), a torch checkpoint without it, and a
  group switched to capturable after a load"""
  from dynibar_amd import optim
  name = 'adamw_amsgrad_maximize'
  cls, kw = OPTION_SETS[name]
  q, opt, grads = check_against_torch(dev, name, capturable=True)
  st = opt.state[q]
  assert st['step'].device == q.device and float(st['step']) == STEPS and st['beta_pow'].dtype == torch.float64
  pw = np.ones(2, D)
  for _ in range(STEPS):
    pw = pow_scalars(LR_TORCH, 0.9, 0.999, pw)[2]
  gc.same64(pw, st['beta_pow'], 'beta_pow after five steps')
  assert pw[1] != D(F(pw[1]))  # (not an fp32 value: a cast would show)
  sd = copy.deepcopy(opt.state_dict())
  q2, opt2, _ = ours_for(dev, name, capturable=True)
  with torch.no_grad():
    q2.copy_(q.detach())
  opt2.load_state_dict(sd)
  s2 = opt2.state[q2]
  assert s2['beta_pow'].dtype == torch.float64 and torch.equal(s2['beta_pow'].cpu(), st['beta_pow'].cpu()) and s2['step'].device == q2.device
  _step(q, opt, grads[STEPS], dev)
  _step(q2, opt2, grads[STEPS], dev)
  assert torch.equal(q.detach(), q2.detach()) and float(opt2.state[q2]['step']) == STEPS + 1
  # torch's own checkpoint (no beta_pow; not capturable), then the group switched to capturable: [beta1 ** t, beta2 ** t] from the host
  ref = torch_reference(name)
  q3, opt3, _ = ours_for(dev, name)
  with torch.no_grad():
    q3.copy_(ref['q32'].detach())
  opt3.load_state_dict(copy.deepcopy(ref['opt32'].state_dict()))
  assert 'beta_pow' not in opt3.state[q3] and opt3.state[q3]['step'].device.type == 'cpu'
  opt3.param_groups[0]['capturable'] = True
  _step(q3, opt3, grads[STEPS], dev)
  s3 = opt3.state[q3]
  assert s3['step'].device == q3.device and float(s3['step']) == STEPS + 1
  gc.same64(pow_scalars(LR_TORCH, 0.9, 0.999, np.array([0.9 ** float(STEPS), 0.999 ** float(STEPS)], D))[2], s3['beta_pow'], 'beta_pow made from a host count')
  # and a capturable checkpoint whose beta_pow is missing (as torch's capturable Adam saves it)
  sd = copy.deepcopy(opt.state_dict())
  for s in sd['state'].values():
    del s['beta_pow']
  q4, opt4, _ = ours_for(dev, name, capturable=True)
  opt4.load_state_dict(sd)
  t = float(STEPS + 1)
  gc.same64(np.array([0.9 ** t, 0.999 ** t], D), opt4.state[q4]['beta_pow'], 'beta_pow of a checkpoint without it')
