"""Support for the tests of the optimizer's guard (dynibar_amd/optim.py, csrc/dyn_optim.h: k_grad_sumsq, k_grad_stats, k_adam_step_guarded,
k_grad_scale): the numpy restatement of the contract of include/dynibar_hip.h -- the chunk sum, the finish, coef and the guarded update -- and
the checks the emulator and the device tests share.  Test infrastructure: nothing in dynibar_amd imports this.

The restatement adds float64 numbers in the kernels' order (lane (e >> 2) & 255, the xor butterfly of a wave, ((w0 + w1) + w2) + w3);
tests/test_optim_guard_cpu.py holds it to the float64 norm and to torch.nn.utils.clip_grad_norm_, and the kernels are compared with it exactly."""
import numpy as np
import torch

import optim_cases as oc

F = np.float32
LANES = 256
_XOR = [np.arange(64) ^ m for m in (32, 16, 8, 4, 2, 1)]


# ---- the contract --------------------------------------------------------------------------------------------------------------------
def block_sum(lanes):
  """[..., 256] lane sums -> [...]: v += shfl_xor(v, m) for m = 32 .. 1 within each wave of 64, then ((w0 + w1) + w2) + w3"""
  v = lanes.reshape(lanes.shape[:-1] + (4, 64))
  for idx in _XOR:
    v = v + v[..., idx]
  w = v[..., 0]
  return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def chunk_sums(g, chunk):
  """the partials of one tensor's chunks, float64 [cdiv(n, chunk)]: element e of a chunk goes to lane (e >> 2) & 255, each lane adds the exact
  squares of its elements in increasing e from 0.0.  (The padding adds exact zeros to sums that are never -0.0: no change.)"""
  g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
  n_chunks = -(-g.size // chunk)
  sq = np.zeros(n_chunks * chunk, np.float64)
  with np.errstate(all='ignore'):
    sq[:g.size] = g.astype(np.float64) * g.astype(np.float64)
    sq = sq.reshape(n_chunks, chunk // (4 * LANES), LANES, 4)
    lanes = np.zeros((n_chunks, LANES), np.float64)
    for r in range(sq.shape[1]):
      for j in range(4):
        lanes = lanes + sq[:, r, :, j]
    return block_sum(lanes)


def finish(partials, max_norm):
  """k_grad_stats -> dict(sumsq, norm, coef, finite); max_norm None or <= 0: no clipping"""
  partials = np.asarray(partials, np.float64)
  rows = -(-partials.size // LANES)
  padded = np.zeros(rows * LANES, np.float64)
  padded[:partials.size] = partials
  with np.errstate(all='ignore'):
    lanes = np.zeros(LANES, np.float64)
    for row in padded.reshape(rows, LANES):
      lanes = lanes + row
    sumsq = np.float64(block_sum(lanes))
    finite = bool(np.isfinite(sumsq))
    norm = F(np.sqrt(sumsq))
    coef = F(1.0)
    if max_norm is not None and max_norm > 0 and finite:
      coef = min(F(1.0), F(max_norm) / (norm + F(1e-6)))
  assert norm.dtype == np.float32 and np.asarray(coef).dtype == np.float32
  return dict(sumsq=sumsq, norm=norm, coef=F(coef), finite=int(finite))


def restate_norm(grads, chunk, max_norm=None):
  """the contract over a list of gradients in table order (None: a record with skip != 0, its chunks store 0.0; ``sizes`` then names its
  size) -> (partials, stats)"""
  parts = [chunk_sums(g, chunk) for g in grads]
  partials = np.concatenate(parts) if parts else np.zeros(0, np.float64)
  return partials, finish(partials, max_norm)


def scaled(g, coef):
  with np.errstate(all='ignore'):
    out = g * F(coef)
  assert out.dtype == np.float32
  return out


def same64(want, got, what):
  got = got.detach().cpu().reshape(-1).to(torch.float64)
  want = torch.from_numpy(np.ascontiguousarray(want, dtype=np.float64).reshape(-1))
  assert want.shape == got.shape, f'{what}: {tuple(got.shape)} values, expected {tuple(want.shape)}'
  assert torch.equal(torch.isnan(want), torch.isnan(got)), f'{what}: NaNs at different places'
  w, g = torch.nan_to_num(want, nan=0.0, posinf=np.inf, neginf=-np.inf), torch.nan_to_num(got, nan=0.0, posinf=np.inf, neginf=-np.inf)
  if not torch.equal(w, g):
    i = int(torch.nonzero(w != g).reshape(-1)[0])
    raise AssertionError(f'{what}: differs, first at {i}: want {float(w[i])!r} got {float(g[i])!r}')


# ---- the harness -----------------------------------------------------------------------------------------------------------------------
class Guarded(oc.Tensors):
  """oc.Tensors whose step is the guarded one: the mirror advances by the restatement of the guard, and every step compares the partial
  sums and the DynGradStats the device wrote with it."""

  def __init__(self, *a, **kw):
    super().__init__(*a, **kw)
    self.calls = self.nonfinite = 0
    self.last = None

  def expect(self, grads, max_grad_norm=None):
    from dynibar_amd import optim
    table = [np.zeros(p.size, np.float32) if g is None else g for g, p in zip(grads, self.p)]  # (a skipped record's chunks store 0.0)
    return restate_norm(table, optim.CHUNK, max_grad_norm)

  def step(self, grads, max_grad_norm=None, skip_nonfinite=False, zero_grads=False, before=None):
    assert max_grad_norm is not None or skip_nonfinite
    partials, st = self.expect(grads, max_grad_norm)
    self.set_grads(grads)
    if before is not None:
      before(self)
    self.opt.step(zero_grads=zero_grads, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
    self.calls += 1
    self.nonfinite += 0 if st['finite'] else 1
    held = skip_nonfinite and not st['finite']
    for i, g in enumerate(grads):
      if g is None:
        continue
      grp = self.opt.param_groups[self.group_of[i]]
      self.t[i] += 1  # (the host's count advances whether or not the device held the step)
      if not held:
        self.p[i], self.m[i], self.v[i] = oc.restate(self.p[i], scaled(g, st['coef']), self.m[i], self.v[i], grp['lr'], grp['betas'][0],
                                                     grp['betas'][1], grp['eps'], self.t[i])
    self.last = st
    self.check_stats(partials, st)
    return st

  def check_stats(self, partials, st):
    seen = self.opt.grad_stats
    assert seen is not None
    for name in ('norm', 'coef', 'finite', 'calls', 'nonfinite'):
      x = getattr(seen, name)
      assert torch.is_tensor(x) and x.dim() == 0 and x.device == self.params[0].device, name
    assert seen.norm.dtype == torch.float32 and seen.coef.dtype == torch.float32
    same64(partials, self.opt._tables['partials'][:len(partials)], 'partials')
    assert self.opt._tables['n_chunks'] == len(partials)
    same64([st['sumsq']], seen.sumsq, 'sumsq')
    oc.same(np.array([st['norm']]), seen.norm, 'norm')
    oc.same(np.array([st['coef']]), seen.coef, 'coef')
    assert int(seen.finite) == st['finite'], ('finite', int(seen.finite), st)
    assert int(seen.calls) == self.calls and int(seen.nonfinite) == self.nonfinite, (int(seen.calls), self.calls, int(seen.nonfinite), self.nonfinite)


def sizes(chunk):
  return [(), 1] + oc.sizes(chunk)[1:]


def _one(shape):
  return [(dict(lr=4e-4), [shape])]


def _around(T, grads):
  """a max_grad_norm below and one above the norm of these gradients"""
  norm = float(T.expect(grads)[1]['norm'])
  assert np.isfinite(norm) and norm > 0
  return 0.5 * norm, 4.0 * norm


# ---- the shared checks ---------------------------------------------------------------------------------------------------------------
def check_single(dev, shape):
  """one tensor from a first-seen parameter: a clipped step (coef < 1), an unclipped one (coef == 1), one with the skip alone"""
  T = Guarded(dev, _one(shape), seed=oc.numel(shape) + 20)
  assert T.opt.grad_stats is None
  g = T.gradients()
  below, above = _around(T, g)
  assert T.step(g, max_grad_norm=below)['coef'] < 1
  T.check()
  g = T.gradients()
  assert T.step(g, max_grad_norm=_around(T, g)[1], skip_nonfinite=True)['coef'] == 1
  T.check()
  assert T.step(T.gradients(), skip_nonfinite=True)['coef'] == 1
  T.check()


def check_misaligned(dev, shape):
  """the same gradient in an aligned view, in views one element off 16 bytes (all four tensors; the gradient alone) and in a plain tensor:
  every chunk's partial is bit-identical across them -- the lane assignment does not depend on the path -- and p, m, v follow the restatement"""
  from dynibar_amd import optim
  offs = {0: (0, 0, 0, 0), 1: (1, 1, 1, 1), 2: (0, 1, 0, 0)}
  T = Guarded(dev, [(dict(lr=4e-4), [shape] * 4)], seed=oc.numel(shape) + 21, offsets=offs)
  per = -(-oc.numel(shape) // optim.CHUNK)
  for clip in (True, False):
    g = T.gradients()[0]
    grads = [g.copy() for _ in range(4)]
    below, above = _around(T, grads)
    T.step(grads, max_grad_norm=below if clip else above, zero_grads=not clip)
    T.check()
    parts = T.opt._tables['partials'].cpu()
    for k in range(1, 4):
      assert torch.equal(parts[:per], parts[k * per:(k + 1) * per]), f'the partials of tensor {k} (offsets {offs.get(k)}) differ from the aligned tensor\'s'
  for i in T.views:
    assert not bool(T.views[i][1].any())


def check_many(dev, chunk):
  """600 tensors in 6 groups and more than 512 chunks: the finish kernel's strided loop takes three rounds.  The second step starts from a
  partials buffer full of NaN and has one tensor in the middle without a gradient."""
  T = Guarded(dev, oc.many_groups(chunk), seed=22)
  assert len(T) == 600
  g = T.gradients()
  T.step(g, max_grad_norm=_around(T, g)[0], skip_nonfinite=True)
  assert T.opt._tables['n_chunks'] > 512
  T.check()
  g = T.gradients()
  g[300] = None
  T.step(g, max_grad_norm=_around(T, g)[0], skip_nonfinite=True, before=lambda t: t.opt._tables['partials'].fill_(float('nan')))
  assert T.t[300] == 1 and T.t[299] == 2
  T.check()


VALUE_CASES = ('zeros', 'subnormals', 'huge')


def check_values(dev, chunk, kind):
  T = Guarded(dev, _one(chunk + 5), seed=23)
  g = T.gradients()
  T.step(g, max_grad_norm=_around(T, g)[0])
  n = T.p[0].size
  for clipped in (True, False):
    if kind == 'zeros':
      g = np.zeros(n, np.float32)
      st = T.step([g], max_grad_norm=1.0 if clipped else None, skip_nonfinite=not clipped)
      assert st['norm'] == 0 and st['coef'] == 1 and st['finite'] == 1
    elif kind == 'subnormals':  # every element below the smallest normal fp32: the squares are exact in double, far below fp32's range
      g = T.rng.integers(1, 2 ** 23, n).astype(np.uint32).view(np.float32) * np.where(T.rng.random(n) < 0.5, F(-1), F(1))
      assert float(np.abs(g).max()) < 1.1754944e-38 and float(np.abs(g).min()) > 0
      st = T.step([g], max_grad_norm=1e-38 if clipped else 1.0)
      assert 0 < st['norm'] < 1e-35 and st['finite'] == 1 and ((st['coef'] < 1) if clipped else (st['coef'] == 1))
    else:  # two elements of 3e38: every gradient is finite, the fp32 norm is not
      g = T.gradients()[0]
      g[[7, chunk + 2]] = F(3e38)
      st = T.step([g], max_grad_norm=1.0 if clipped else None, skip_nonfinite=True)
      assert st['finite'] == 1 and np.isinf(st['norm']) and st['coef'] == (0 if clipped else 1)
    T.check()
    assert int(T.opt.grad_stats.nonfinite) == 0
  T.step(T.gradients(), max_grad_norm=1.0)  # what the case left in the moments goes through a further step
  T.check()


NONFINITE_CASES = [(value, mode) for value in ('nan', 'inf') for mode in ('skip', 'skip_zero', 'propagate')]


def check_nonfinite(dev, chunk, value, mode):
  """after two warm steps one gradient element in the last chunk of the largest tensor is NaN / Inf"""
  T = Guarded(dev, [(dict(lr=4e-4), [37, 2 * chunk + 5]), (dict(lr=1e-3), [(), 300])], seed=24)
  for _ in range(2):
    g = T.gradients()
    T.step(g, max_grad_norm=_around(T, g)[0], skip_nonfinite=True)
  T.check()
  held = [(x.detach().clone(), T.opt.state[x]['exp_avg'].clone(), T.opt.state[x]['exp_avg_sq'].clone()) for x in T.params]
  g = T.gradients()
  g[1][2 * chunk + 3] = np.nan if value == 'nan' else np.inf
  st = T.step(g, max_grad_norm=1.0, skip_nonfinite=mode != 'propagate', zero_grads=mode == 'skip_zero')
  assert st['finite'] == 0 and st['coef'] == 1 and T.calls == 3 and T.nonfinite == 1
  assert int(T.opt.grad_stats.calls) == 3 and int(T.opt.grad_stats.nonfinite) == 1
  T.check()
  assert T.t == [3, 3, 3, 3] and all(float(T.opt.state[x]['step']) == 3.0 for x in T.params)  # the host's counts advanced
  if mode == 'propagate':
    bad = T.params[1].detach().reshape(-1)
    assert bool(torch.isnan(bad[2 * chunk + 3])) and int(torch.isnan(bad).sum()) == 1
    assert all(bool(torch.isfinite(T.params[i]).all()) for i in (0, 2, 3))
    return
  for x, (p0, m0, v0) in zip(T.params, held):  # bitwise as they were
    assert torch.equal(x.detach(), p0) and torch.equal(T.opt.state[x]['exp_avg'], m0) and torch.equal(T.opt.state[x]['exp_avg_sq'], v0)
  if mode == 'skip_zero':
    assert all(x.grad is not None and not bool(x.grad.any()) for x in T.params)
  else:
    assert bool(torch.isnan(T.params[1].grad).any() if value == 'nan' else torch.isinf(T.params[1].grad).any())  # .grad is left alone
  g = T.gradients()
  T.step(g, max_grad_norm=_around(T, g)[0], skip_nonfinite=True, zero_grads=mode == 'skip_zero')  # a clean step with the advanced t = 4
  assert T.t == [4, 4, 4, 4] and T.last['finite'] == 1 and T.nonfinite == 1
  T.check()


def check_steplr(dev, chunk):
  """ten guarded steps under StepLR, then the state through torch.optim.Adam and back, then one more guarded step"""
  from dynibar_amd import optim
  T = Guarded(dev, [(dict(lr=4e-4), [chunk + 1, 5]), (dict(lr=1e-3), [33])], seed=25)
  sched = torch.optim.lr_scheduler.StepLR(T.opt, step_size=3, gamma=0.5)
  for s in range(10):
    g = T.gradients()
    below, above = _around(T, g)
    T.step(g, max_grad_norm=below if s % 2 == 0 else above, skip_nonfinite=True)
    sched.step()
  assert T.opt.param_groups[0]['lr'] == 4e-4 * 0.5 ** 3 and T.opt.param_groups[1]['lr'] == 1e-3 * 0.5 ** 3
  T.check()
  theirs = torch.optim.Adam([dict(params=T.params[:2]), dict(params=T.params[2:])])
  theirs.load_state_dict(T.opt.state_dict())
  for x in T.params:
    assert float(theirs.state[x]['step']) == 10.0 and torch.equal(theirs.state[x]['exp_avg'], T.opt.state[x]['exp_avg'])
  back = optim.Adam([dict(params=T.params[:2]), dict(params=T.params[2:])])
  back.load_state_dict(theirs.state_dict())
  assert back.grad_stats is None
  T.opt = back
  g = T.gradients()
  T.calls = T.nonfinite = 0  # (a new optimizer: new tables, counters from zero)
  T.step(g, max_grad_norm=_around(T, g)[0], skip_nonfinite=True)
  assert T.t == [11, 11, 11]
  T.check()


def check_standalone(dev, chunk):
  """grad_norm and clip_grad_norm_ on their own: one non-contiguous gradient, one parameter without a gradient"""
  from dynibar_amd import optim
  import pytest
  T = Guarded(dev, [(dict(lr=4e-4), [chunk + 9, (5, 7), (), 40])], seed=26, noncontiguous_grads={1})
  grads = T.gradients()
  grads[3] = None
  T.set_grads(grads)
  have = [g for g in grads if g is not None]
  partials, st = restate_norm(have, optim.CHUNK)
  norm = optim.grad_norm(T.params)
  assert norm.dim() == 0 and norm.dtype == torch.float32 and norm.device == T.params[0].device
  oc.same(np.array([st['norm']]), norm, 'grad_norm')
  for x, g in zip(T.params, grads):
    if g is not None:
      oc.same(g, x.grad, 'grad_norm leaves .grad alone')
  # unclipped: .grad stays bit for bit; clipped: g * coef, the strided gradient included
  for max_norm, clipped in ((4.0 * float(st['norm']), False), (0.5 * float(st['norm']), True)):
    want = finish(partials, max_norm)
    assert (want['coef'] < 1) == clipped
    got = optim.clip_grad_norm_(T.params, max_norm)
    oc.same(np.array([want['norm']]), got, 'the norm clip_grad_norm_ returns')
    for i, (x, g) in enumerate(zip(T.params, grads)):
      if g is None:
        assert x.grad is None
      else:
        oc.same(scaled(g, want['coef']), x.grad, f'.grad of tensor {i} after clip_grad_norm_')
    assert not T.params[1].grad.is_contiguous()
  oc.same(np.array([st['norm']]), norm, 'an earlier result is the caller\'s own')
  # the same gradients through the optimizer: grad_stats.norm is grad_norm, bit for bit
  T.set_grads(grads)
  alone = optim.grad_norm(T.params)
  T.step(grads, skip_nonfinite=True)
  assert torch.equal(alone, T.opt.grad_stats.norm)
  # a single tensor, nothing to do, and the non-finite error
  T.set_grads(grads)
  oc.same(np.array([restate_norm([grads[0]], optim.CHUNK)[1]['norm']]), optim.grad_norm(T.params[0]), 'grad_norm of one tensor')
  zero = optim.clip_grad_norm_([], 1.0)
  assert zero.dim() == 0 and float(zero) == 0.0 and float(optim.grad_norm([T.params[3]])) == 0.0
  grads[0][chunk + 3] = np.inf
  T.set_grads(grads)
  with pytest.raises(RuntimeError, match='non-finite'):
    optim.clip_grad_norm_(T.params, 1.0, error_if_nonfinite=True)
  got = optim.clip_grad_norm_(T.params, 1.0)  # without the error: coef stays 1, the gradients stay as they are
  assert bool(torch.isinf(got))
  for x, g in zip(T.params, grads):
    if g is not None:
      oc.same(g, x.grad, '.grad after a non-finite clip')
