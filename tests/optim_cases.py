"""Support for the optimizer tests (dynibar_amd/optim.py, csrc/dyn_optim.h): the numpy restatement of the update contract of
include/dynibar_hip.h, seeded gradients, a harness that keeps a numpy mirror of an optimizer's tensors, and the checks the CPU, the emulator and
the device tests share.  Test infrastructure: nothing in dynibar_amd imports this.

The restatement is fp32 numpy, one rounding per operation; tests/test_optim_cpu.py bounds its distance from a float64 ``torch.optim.Adam`` by the
distance of torch's own fp32 Adam, and the kernel is compared with the restatement exactly (torch.equal; NaNs by position)."""
import math

import numpy as np
import torch

F = np.float32
SENTINEL = 7.25   # what the flat buffers hold around a view
LEAD = 4          # floats in front of a view at offset 0: the view then starts on 16 bytes
PAD = 16          # floats a flat buffer is longer than its view
# (p, g, m, v) offsets in floats from a 16-byte boundary: the float4 path, each pointer alone off it, all of them by different and by equal amounts
OFFSETS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (1, 2, 3, 3), (2, 2, 2, 2)]


def sizes(chunk):
  return [(), 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]


def numel(shape):
  return int(np.prod(shape, dtype=np.int64)) if isinstance(shape, tuple) else int(shape)


# ---- the contract --------------------------------------------------------------------------------------------------------------------
def scalars(lr, beta1, beta2, t):
  """(a, s2): Python double, rounded to fp32 once"""
  return F(-lr / (1 - beta1 ** t)), F(math.sqrt(1 - beta2 ** t))


def restate(p, g, m, v, lr, beta1, beta2, eps, t):
  """one step of the contract on fp32 arrays -> (p, m, v); t is the step count after the increment"""
  assert p.dtype == g.dtype == m.dtype == v.dtype == np.float32
  a, s2 = scalars(lr, beta1, beta2, t)
  c1, c2, b2, e = F(1 - beta1), F(1 - beta2), F(beta2), F(eps)
  with np.errstate(all='ignore'):
    m = m + c1 * (g - m)
    v = v * b2 + (c2 * g) * g
    denom = np.sqrt(v) / s2 + e
    p = p + (a * m) / denom
  assert p.dtype == m.dtype == v.dtype == np.float32
  return p, m, v


def gradient(rng, n):
  """a standard normal times 10^k, k drawn per element from -6..1"""
  return (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2, n)).astype(np.float32)


def same(want, got, what):
  """exact equality of a numpy array and a tensor; NaNs must sit at the same places (their payloads are not compared)"""
  got = got.detach().cpu().reshape(-1)
  want = torch.from_numpy(np.ascontiguousarray(want, dtype=np.float32).reshape(-1))
  assert torch.equal(torch.isnan(want), torch.isnan(got)), f'{what}: NaNs at different places'
  w, g = torch.where(torch.isnan(want), torch.zeros_like(want), want), torch.where(torch.isnan(got), torch.zeros_like(got), got)
  if not torch.equal(w, g):
    bad = torch.nonzero(w != g).reshape(-1)
    i = int(bad[0])
    raise AssertionError(f'{what}: {bad.numel()} of {w.numel()} elements differ, first at {i}: want {float(w[i])!r} got {float(g[i])!r}')


# ---- the harness -----------------------------------------------------------------------------------------------------------------------
class Tensors:
  """The tensors of one ``optim.Adam`` on ``dev`` and their numpy mirror, advanced by the restatement.
  groups: [(options, [shape, ...])], a shape an int n or a tuple.  offsets: {tensor index: (p, g, m, v) offsets} -- such a tensor, its gradient
  and its moments are views into flat buffers full of SENTINEL, and it starts from a loaded state (t = 2, random moments)."""

  def __init__(self, dev, groups, seed=0, offsets=None, noncontiguous_grads=()):
    from dynibar_amd import optim
    self.dev, self.rng = dev, np.random.default_rng([seed, 77])
    self.shapes, self.group_of, self.params, self.flats, self.views = [], [], [], {}, {}
    self.p, self.m, self.v, self.t = [], [], [], []
    self.noncontiguous = set(noncontiguous_grads)
    offsets = offsets or {}
    arg, preload = [], {}
    for gi, (opts, shapes) in enumerate(groups):
      ps = []
      for shape in shapes:
        i, n = len(self.params), numel(shape)
        tshape = shape if isinstance(shape, tuple) else (shape,)
        p0 = self.rng.standard_normal(n).astype(np.float32)
        self.p.append(p0)
        if i in offsets:
          m0 = (0.1 * self.rng.standard_normal(n)).astype(np.float32)
          v0 = (0.01 * self.rng.standard_normal(n) ** 2).astype(np.float32)
          t0 = 2
          views = []
          for off, init in zip(offsets[i], (p0, np.zeros(n, np.float32), m0, v0)):
            flat = torch.full((n + PAD,), SENTINEL, dtype=torch.float32, device=dev)
            view = flat[LEAD + off:LEAD + off + n]
            view.copy_(torch.from_numpy(init))
            views.append(view.view(tshape))
            assert (view.data_ptr() % 16 == 0) == (off == 0)
          self.flats[i], self.views[i] = [v_._base if v_._base is not None else v_ for v_ in views], views
          param = torch.nn.Parameter(views[0])
          preload[i] = (param, views[2], views[3], t0)
        else:
          m0, v0, t0 = np.zeros(n, np.float32), np.zeros(n, np.float32), 0
          param = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dev).view(tshape))
        self.m.append(m0); self.v.append(v0); self.t.append(t0)
        self.shapes.append(tshape); self.group_of.append(gi); self.params.append(param)
        ps.append(param)
      arg.append(dict(params=ps, **opts))
    self.opt = optim.Adam(arg)
    for i, (param, mv, vv, t0) in preload.items():
      self.opt.state[param] = dict(step=torch.tensor(float(t0), dtype=torch.float32), exp_avg=mv, exp_avg_sq=vv)

  def __len__(self):
    return len(self.params)

  def gradients(self, which=None):
    """a seeded gradient for every tensor (``which``: only those indices, None elsewhere)"""
    return [gradient(self.rng, p.size) if which is None or i in which else None for i, p in enumerate(self.p)]

  def set_grads(self, grads):
    for i, (param, g) in enumerate(zip(self.params, grads)):
      if g is None:
        param.grad = None
      elif i in self.views:
        self.views[i][1].copy_(torch.from_numpy(g).view(self.shapes[i]))
        param.grad = self.views[i][1]
      elif i in self.noncontiguous:
        r, c = self.shapes[i]
        param.grad = torch.from_numpy(np.ascontiguousarray(g.reshape(r, c).T)).to(self.dev).T
        assert not param.grad.is_contiguous()
      else:
        param.grad = torch.from_numpy(g.copy()).to(self.dev).view(self.shapes[i])

  def step(self, grads, **kw):
    """the optimizer's step on the device and the restatement's on the mirror, with each group's lr as it is now"""
    self.set_grads(grads)
    self.opt.step(**kw)
    for i, g in enumerate(grads):
      if g is None:
        continue
      grp = self.opt.param_groups[self.group_of[i]]
      self.t[i] += 1
      self.p[i], self.m[i], self.v[i] = restate(self.p[i], g, self.m[i], self.v[i], grp['lr'], grp['betas'][0], grp['betas'][1], grp['eps'], self.t[i])

  def adopt(self):
    """take the mirror from the optimizer's tensors as they are (after load_state_dict)"""
    for i, param in enumerate(self.params):
      self.p[i] = param.detach().cpu().numpy().reshape(-1).copy()
      st = self.opt.state.get(param)
      if st:
        self.m[i] = st['exp_avg'].cpu().numpy().reshape(-1).copy()
        self.v[i] = st['exp_avg_sq'].cpu().numpy().reshape(-1).copy()
        self.t[i] = int(st['step'])

  def check(self):
    for i, param in enumerate(self.params):
      same(self.p[i], param, f'p of tensor {i} {self.shapes[i]}')
      st = self.opt.state.get(param)
      if self.t[i] == 0:
        assert not st, f'tensor {i} never had a gradient but has state {list(st)}'
        continue
      assert st['step'].dtype == torch.float32 and st['step'].device.type == 'cpu' and st['step'].dim() == 0
      assert float(st['step']) == self.t[i], f'tensor {i}: step {float(st["step"])} != {self.t[i]}'
      assert st['exp_avg'].shape == param.shape and st['exp_avg'].device == param.device
      same(self.m[i], st['exp_avg'], f'm of tensor {i} {self.shapes[i]}')
      same(self.v[i], st['exp_avg_sq'], f'v of tensor {i} {self.shapes[i]}')
    for i, flats in self.flats.items():
      n = self.p[i].size
      for flat, view, name in zip(flats, self.views[i], 'pgmv'):
        off = view.storage_offset()
        outside = torch.cat([flat[:off], flat[off + n:]]).cpu()
        assert outside.numel() == PAD and torch.equal(outside, torch.full((PAD,), SENTINEL)), f'tensor {i}: {name} was written outside its view'


def _one(shape):
  return [(dict(lr=4e-4), [shape])]


# ---- the shared checks ---------------------------------------------------------------------------------------------------------------
def check_single(dev, shape):
  """one launch over one tensor, three steps from a first-seen parameter"""
  T = Tensors(dev, _one(shape), seed=numel(shape))
  for _ in range(3):
    T.step(T.gradients())
  T.check()


def check_misaligned(dev, shape):
  """seven tensors of one size in one launch, as views at OFFSETS: the float4 path, the scalar path and both in one grid"""
  T = Tensors(dev, [(dict(lr=4e-4), [shape] * len(OFFSETS))], seed=numel(shape) + 1, offsets=dict(enumerate(OFFSETS)))
  for _ in range(2):
    T.step(T.gradients())
  T.check()
  T.step(T.gradients(), zero_grads=True)  # (the fused clearing must stay inside the views as well)
  T.check()
  for i in T.views:
    assert not bool(T.views[i][1].any())


def many_groups(chunk):
  rng = np.random.default_rng(600)
  pool = [(), 1, 2, 3, 5, 31, 64, 100, 257, 1023, (3, 7), (16, 4, 3)]
  groups = []
  for gi, lr in enumerate((4e-4, 1e-3, 5e-4, 2e-4, 1e-3, 1e-4)):
    opts = dict(lr=lr)
    if gi == 2:
      opts.update(betas=(0.8, 0.99), eps=1e-6)
    shapes = [pool[int(k)] for k in rng.integers(0, len(pool), 100)]
    shapes[gi * 7 % 100] = (chunk + 1, chunk, 2 * chunk + 5, chunk - 1, 3 * chunk, chunk + 3)[gi]
    groups.append((opts, shapes))
  return groups


def check_many(dev, chunk):
  """600 tensors of mixed sizes in 6 groups with their own lr (one with its own betas and eps), one launch per step"""
  T = Tensors(dev, many_groups(chunk), seed=6)
  assert len(T) == 600
  for _ in range(2):
    T.step(T.gradients())
  T.check()


def check_grad_none_between(dev, chunk):
  T = Tensors(dev, [(dict(lr=4e-4), [chunk + 1, 37, 9])], seed=3)
  T.step(T.gradients())
  before = [x.copy() for x in (T.p[1], T.m[1], T.v[1])]
  st = T.opt.state[T.params[1]]
  held = [T.params[1].detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone()]
  for _ in range(2):
    T.step(T.gradients(which={0, 2}))
  T.check()
  assert T.t == [3, 1, 3] and float(st['step']) == 1.0
  for w, h, now in zip(before, held, (T.params[1], st['exp_avg'], st['exp_avg_sq'])):
    same(w, now, 'the tensor without a gradient')
    assert torch.equal(h, now.detach())


def check_late_first_gradient(dev, chunk):
  """tensor 1 first receives a gradient at step 4: t = 4, 1, 4 inside one launch, and it starts from zero moments"""
  T = Tensors(dev, [(dict(lr=1e-3), [130, chunk + 7]), (dict(lr=4e-4), [11])], seed=4)
  for s in range(6):
    T.step(T.gradients(which=None if s >= 3 else {0, 2}))
    if s == 2:
      assert T.params[1] not in T.opt.state or not T.opt.state[T.params[1]]
  assert T.t == [6, 3, 6]
  T.check()


def check_lr_zero(dev):
  T = Tensors(dev, [(dict(lr=4e-4), [50]), (dict(lr=0.0), [70, ()])], seed=5)
  start = [T.params[i].detach().clone() for i in (1, 2)]
  for _ in range(2):
    T.step(T.gradients())
  T.check()
  for i, s in zip((1, 2), start):
    assert torch.equal(s, T.params[i].detach())  # lr = 0: the parameter stays, bit for bit
    st = T.opt.state[T.params[i]]
    assert float(st['step']) == 2.0 and bool(st['exp_avg'].abs().sum() > 0) and bool(st['exp_avg_sq'].sum() > 0)


VALUE_CASES = ('zeros', 'tiny_huge', 'nan')


def check_values(dev, chunk, kind):
  T = Tensors(dev, _one(chunk + 5), seed=8)
  T.step(T.gradients())
  g = T.gradients()[0]
  if kind == 'zeros':
    g[:] = 0.0
  elif kind == 'tiny_huge':  # 1e-20: (c2 g) g = 1e-43 is subnormal; 1e20: g * g would overflow
    g[[0, 5, chunk - 1, chunk + 4]] = F(1e-20)
    g[[1, 6, chunk, chunk + 3]] = F(1e20)
    g[[2, 7]] = F(-1e20)
    g[3] = F(1e-45)
  else:
    g[chunk + 2] = np.nan
  T.step([g])
  T.check()
  T.step(T.gradients())  # what the case left in the moments (inf, NaN, subnormals) goes through a further step
  T.check()
  if kind == 'nan':
    assert int(torch.isnan(T.params[0]).sum()) == 1
  if kind == 'tiny_huge':
    assert bool(torch.isfinite(T.params[0]).all())  # (g * g overflows; the contract's (c2 g) g = 1e37 does not)


def check_steplr(dev, chunk):
  T = Tensors(dev, [(dict(lr=4e-4), [chunk + 1, 5]), (dict(lr=1e-3), [33])], seed=9)
  sched = torch.optim.lr_scheduler.StepLR(T.opt, step_size=3, gamma=0.5)
  for _ in range(10):
    T.step(T.gradients())
    sched.step()
  assert T.opt.param_groups[0]['lr'] == 4e-4 * 0.5 ** 3 and T.opt.param_groups[1]['lr'] == 1e-3 * 0.5 ** 3
  T.check()


def check_loaded_state(dev, chunk):
  """three steps of torch.optim.Adam on the host, its state_dict loaded here, three more steps against the restatement continued from the same numbers"""
  groups = [(dict(lr=4e-4), [chunk + 1, ()]), (dict(lr=1e-3, betas=(0.85, 0.995)), [19])]
  T = Tensors(dev, groups, seed=10)
  host = [torch.nn.Parameter(torch.from_numpy(p.copy()).view(s)) for p, s in zip(T.p, T.shapes)]
  topt = torch.optim.Adam([dict(params=host[:2], **groups[0][0]), dict(params=host[2:], **groups[1][0])])
  for _ in range(3):
    for h, g in zip(host, T.gradients()):
      h.grad = torch.from_numpy(g).view(h.shape)
    topt.step()
  with torch.no_grad():
    for param, h in zip(T.params, host):
      param.copy_(h)
  T.opt.load_state_dict(topt.state_dict())
  T.adopt()
  assert T.t == [3, 3, 3]
  for i, h in enumerate(host):
    same(topt.state[h]['exp_avg'].numpy(), T.opt.state[T.params[i]]['exp_avg'], 'the loaded exp_avg')
    assert T.opt.state[T.params[i]]['exp_avg'].device == T.params[i].device
  for _ in range(3):
    T.step(T.gradients())
  T.check()


class Ops(torch.utils._python_dispatch.TorchDispatchMode):
  """the aten calls made under it"""

  def __init__(self):
    super().__init__()
    self.seen = []

  def __torch_dispatch__(self, func, types, args=(), kwargs=None):
    self.seen.append(str(func))
    return func(*args, **(kwargs or {}))


def check_zero_grads(dev, chunk):
  groups = [(dict(lr=4e-4), [chunk + 9, (5, 7), ()]), (dict(lr=1e-3), [40])]
  A, B = (Tensors(dev, groups, seed=11, noncontiguous_grads={1}) for _ in range(2))
  for _ in range(2):
    grads = A.gradients()
    B.gradients()
    A.step(grads)
    B.step(grads, zero_grads=True)
    for pa, pb, g in zip(A.params, B.params, grads):
      same(g, pa.grad.contiguous(), 'the default form leaves .grad alone')
      assert pb.grad is not None and not bool(pb.grad.any()), 'zero_grads=True: the gradient reads zero afterwards'
  A.check()
  B.check()
  for pa, pb in zip(A.params, B.params):
    assert torch.equal(pa.detach(), pb.detach())
    for key in ('exp_avg', 'exp_avg_sq'):
      assert torch.equal(A.opt.state[pa][key], B.opt.state[pb][key])
  kept = [p.grad for p in B.params]
  with Ops() as ops:
    B.opt.zero_grad(set_to_none=False)
  assert [f for f in ops.seen if 'detach' not in f] == [], ops.seen  # nothing left to clear: no fill, no kernel
  assert all(p.grad is k for p, k in zip(B.params, kept))
  B.params[0].grad.add_(1.0)  # a gradient written since (a backward pass accumulates in place) is cleared the usual way
  B.opt.zero_grad(set_to_none=False)
  assert not bool(B.params[0].grad.any())
  A.opt.zero_grad(set_to_none=False)  # and without the fused clearing zero_grad is torch's
  assert all(not bool(p.grad.any()) for p in A.params)
  B.opt.zero_grad()
  assert all(p.grad is None for p in B.params)


def check_tensor_refusals(dev):
  """what step() refuses about a tensor, before anything is launched or counted: the other tensor of the group stays as it is"""
  from dynibar_amd import optim

  def attempt(bad, exc, match):
    good = torch.nn.Parameter(torch.ones(6, device=dev))
    good.grad = torch.ones(6, device=dev)
    opt = optim.Adam([good, bad], lr=1e-2)
    import pytest
    with pytest.raises(exc, match=match):
      opt.step()
    assert torch.equal(good.detach().cpu(), torch.ones(6)) and not opt.state.get(good)

  p = torch.nn.Parameter(torch.ones(4, dtype=torch.float64, device=dev))
  p.grad = torch.ones(4, dtype=torch.float64, device=dev)
  attempt(p, TypeError, 'float64')
  p = torch.nn.Parameter(torch.ones(4, dtype=torch.float16, device=dev))
  attempt(p, TypeError, 'float16')  # (refused with or without a gradient)
  p = torch.nn.Parameter(torch.ones(4, 6, device=dev).t())
  p.grad = torch.ones(6, 4, device=dev)
  attempt(p, ValueError, 'not contiguous')
  p = torch.nn.Parameter(torch.ones(4, 3, device=dev))
  p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3)).to(dev)
  attempt(p, RuntimeError, 'sparse')
  p = torch.nn.Parameter(torch.ones(4, 3, device=dev))
  p.grad = torch.ones(4, 3, device=dev)
  p.data = torch.ones(5, 3, device=dev)  # (torch refuses a mismatched .grad on assignment; a parameter re-pointed afterwards gets past it)
  attempt(p, ValueError, r'gradient of parameter 1 of group 0 \(5, 3\) is \(4, 3\)')
