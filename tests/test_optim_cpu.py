"""Host-side checks of the optimizer (dynibar_amd/optim.py, csrc/dyn_optim.h): the yardstick itself -- the numpy restatement of the update
contract against torch.optim.Adam in float64 --, the exchange of state_dicts with torch.optim.Adam in both directions, and every refusal that
needs no launch.  No kernel runs here; the kernel is compared with the restatement in tests/emu/test_emu_optim.py and tests/test_gpu_optim.py."""
import copy

import numpy as np
import pytest
import torch

import optim_cases as oc
from dynibar_amd import optim

ALLOWED = dict(p=2.0, v=2.0, m=4.0)  # the multiple of torch's own fp32 distance from float64 the restatement may have (m: torch fuses its lerp)


def _torch_adam(p0, dtype):
  p = torch.nn.Parameter(torch.from_numpy(p0).to(dtype))
  return p, torch.optim.Adam([p], lr=4e-4)


@pytest.mark.parametrize('n', [1, 3, 129, 4097, 70001])
def test_restatement_is_as_close_to_float64_as_torch_fp32(n):
  """200 steps, lr 4e-4, gradients a standard normal times 10^k with k from -6..1 per element, every 17th step all zeros.  The worst distance
  over all steps of the restatement from torch.optim.Adam in float64, against the worst distance of torch's own fp32 CPU Adam on the same
  data: p plain, m over the running max |g|, v over its square."""
  rng = np.random.default_rng([n, 200])
  p0 = rng.standard_normal(n).astype(np.float32)
  p64, o64 = _torch_adam(p0, torch.float64)
  p32, o32 = _torch_adam(p0, torch.float32)
  p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
  worst = {k: dict(restatement=0.0, torch=0.0) for k in 'pmv'}
  gmax = 0.0
  for t in range(1, 201):
    g = np.zeros(n, np.float32) if t % 17 == 0 else oc.gradient(rng, n)
    gmax = max(gmax, float(np.abs(g).max()))
    p64.grad, p32.grad = torch.from_numpy(g).double(), torch.from_numpy(g.copy())
    o64.step()
    o32.step()
    p, m, v = oc.restate(p, g, m, v, 4e-4, 0.9, 0.999, 1e-8, t)
    if gmax == 0.0:
      continue
    ref = dict(p=p64.detach().numpy(), m=o64.state[p64]['exp_avg'].numpy(), v=o64.state[p64]['exp_avg_sq'].numpy())
    tor = dict(p=p32.detach().numpy(), m=o32.state[p32]['exp_avg'].numpy(), v=o32.state[p32]['exp_avg_sq'].numpy())
    for k, mine, scale in (('p', p, 1.0), ('m', m, gmax), ('v', v, gmax * gmax)):
      worst[k]['restatement'] = max(worst[k]['restatement'], float(np.abs(mine.astype(np.float64) - ref[k]).max()) / scale)
      worst[k]['torch'] = max(worst[k]['torch'], float(np.abs(tor[k].astype(np.float64) - ref[k]).max()) / scale)
  for k in 'pvm':
    w = worst[k]
    print(f'  n={n:6d} {k}: restatement {w["restatement"]:.3e}  torch fp32 {w["torch"]:.3e}  ratio {w["restatement"] / w["torch"] if w["torch"] else float("nan"):.3f}'
          f' (allowed {ALLOWED[k]:g})')
  for k in 'pvm':
    assert worst[k]['restatement'] <= ALLOWED[k] * worst[k]['torch'], (n, k, worst[k])


def test_scalars_are_torchs():
  """the per-step scalars of the package equal the restatement's, and step counts read back from float32 tensors are the integers"""
  for lr, b1, b2 in ((4e-4, 0.9, 0.999), (1e-3, 0.85, 0.995), (0.0, 0.9, 0.999)):
    for t in (1, 2, 3, 17, 1000, 250000):
      a, s2 = optim.step_scalars(lr, b1, b2, torch.tensor(float(t), dtype=torch.float32).item())
      wa, ws2 = oc.scalars(lr, b1, b2, t)
      assert a.dtype == np.float32 and s2.dtype == np.float32 and a == wa and s2 == ws2
  assert optim.CHUNK >= 256 and optim.CHUNK % 4 == 0
  assert optim.RECORD.itemsize == 72 and optim.RECORD.fields['n'][1] == 32


def _host_model(seed=0):
  g = torch.Generator().manual_seed(seed)
  return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((7, 3), (5,), (), (2, 3, 4))]


def _six(ps, cls):
  """two groups the way ibrnet/model.py:341-364 writes them, the bare-tensor group included"""
  return cls([{'params': ps[:2], 'lr': 4e-4}, {'params': ps[2], 'lr': 1e-3}, {'params': ps[3:], 'lr': 5e-4, 'betas': (0.8, 0.99)}], lr=2e-4, eps=1e-7)


def _torch_steps(ps, opt, k, seed):
  g = torch.Generator().manual_seed(seed)
  for _ in range(k):
    for p in ps:
      p.grad = torch.randn(p.shape, generator=g)
    opt.step()


def _assert_same_state_dict(a, b):
  assert a['param_groups'] == b['param_groups']
  assert a['state'].keys() == b['state'].keys()
  for k in a['state']:
    assert a['state'][k].keys() == b['state'][k].keys()
    for name in a['state'][k]:
      x, y = a['state'][k][name], b['state'][k][name]
      assert x.dtype == y.dtype and x.device == y.device and x.shape == y.shape and torch.equal(x, y), (k, name)


def test_constructor_is_torchs():
  ps = _host_model()
  ours, theirs = _six(ps, optim.Adam), _six(ps, torch.optim.Adam)
  assert isinstance(ours, torch.optim.Optimizer)
  assert ours.state_dict() == theirs.state_dict()  # (no state yet: the groups, every key and value)
  assert ours.defaults == theirs.defaults
  assert [g['lr'] for g in ours.param_groups] == [4e-4, 1e-3, 5e-4] and ours.param_groups[2]['betas'] == (0.8, 0.99)
  ours.add_param_group({'params': [torch.nn.Parameter(torch.zeros(3))], 'lr': 1e-5})
  assert len(ours.param_groups) == 4 and ours.param_groups[3]['eps'] == 1e-7
  for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0))):
    with pytest.raises(ValueError):
      optim.Adam(_host_model(), **kw)


def test_state_dict_goes_both_ways():
  ps = _host_model()
  theirs = _six(ps, torch.optim.Adam)
  _torch_steps(ps, theirs, 3, 1)
  sd = copy.deepcopy(theirs.state_dict())
  # torch -> this class
  mine = [torch.nn.Parameter(p.detach().clone()) for p in ps]
  ours = _six(mine, optim.Adam)
  ours.load_state_dict(copy.deepcopy(sd))
  _assert_same_state_dict(ours.state_dict(), sd)
  for p in mine:
    st = ours.state[p]
    assert st['step'].dtype == torch.float32 and st['step'].device.type == 'cpu' and st['step'].dim() == 0 and float(st['step']) == 3.0
    assert st['exp_avg'].shape == p.shape and st['exp_avg_sq'].dtype == torch.float32
  # this class -> torch: an optimizer that loads what this class saved continues exactly like the one that was saved
  back = [torch.nn.Parameter(p.detach().clone()) for p in ps]
  again = _six(back, torch.optim.Adam)
  again.load_state_dict(copy.deepcopy(ours.state_dict()))
  _assert_same_state_dict(again.state_dict(), sd)
  _torch_steps(ps, theirs, 2, 2)
  _torch_steps(back, again, 2, 2)
  for p, q in zip(ps, back):
    assert torch.equal(p.detach(), q.detach())
  # a scheduler's lr travels with the groups
  torch.optim.lr_scheduler.StepLR(ours, step_size=1, gamma=0.5)
  assert ours.param_groups[0]['initial_lr'] == 4e-4


def test_integer_step_of_an_old_checkpoint():
  """torch 1.10 saved 'step' as a Python int and groups of lr, betas, eps, weight_decay, amsgrad alone"""
  ps = _host_model()
  theirs = _six(ps, torch.optim.Adam)
  _torch_steps(ps, theirs, 3, 1)
  sd = copy.deepcopy(theirs.state_dict())
  for st in sd['state'].values():
    st['step'] = int(st['step'])
  sd['param_groups'] = [{k: g[k] for k in ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'params')} for g in sd['param_groups']]
  ours = _six([torch.nn.Parameter(p.detach().clone()) for p in ps], optim.Adam)
  ours.load_state_dict(sd)
  for g in ours.param_groups:
    assert g['maximize'] is False and g['capturable'] is False and g['foreach'] is None and g['fused'] is None
    for p in g['params']:
      s = ours.state[p]['step']
      assert torch.is_tensor(s) and s.dtype == torch.float32 and s.device.type == 'cpu' and float(s) == 3.0
  fresh = _six([torch.nn.Parameter(p.detach().clone()) for p in ps], torch.optim.Adam)
  fresh.load_state_dict(ours.state_dict())  # and on to today's torch
  assert all(float(fresh.state[p]['step']) == 3.0 for g in fresh.param_groups for p in g['params'])


def test_unbuilt_options_are_refused_by_name():
  for kw, match in ((dict(amsgrad=True), 'amsgrad'), (dict(maximize=True), 'maximize'), (dict(weight_decay=1e-4), 'weight_decay'),
                    (dict(capturable=True), 'capturable'), (dict(differentiable=True), 'differentiable'), (dict(foreach=False), 'foreach'),
                    (dict(foreach=True), 'foreach'), (dict(fused=False), 'fused'), (dict(fused=True), 'fused')):
    with pytest.raises(NotImplementedError, match=match):
      optim.Adam(_host_model(), **kw)
  with pytest.raises(NotImplementedError, match='weight_decay'):
    optim.Adam([{'params': _host_model(), 'weight_decay': 0.1}])
  with pytest.raises(ValueError, match='lr must be a number'):
    optim.Adam(_host_model(), lr=torch.tensor(1e-3))
  ours = optim.Adam(_host_model())
  ours.param_groups[0]['amsgrad'] = True  # (as a loaded checkpoint may set it)
  with pytest.raises(NotImplementedError, match=r'amsgrad=True \(group 0\)'):
    ours.step()


def test_tensors_are_refused_before_a_launch():
  oc.check_tensor_refusals('cpu')


def test_host_tensors_are_refused():
  """there is no CPU fallback: a step on host parameters raises and changes nothing"""
  ps = _host_model()
  ours = optim.Adam(ps, lr=1e-2)
  for p in ps:
    p.grad = torch.ones_like(p)
  before = [p.detach().clone() for p in ps]
  with pytest.raises(RuntimeError, match='HIP device'):
    ours.step()
  assert all(torch.equal(b, p.detach()) for b, p in zip(before, ps)) and len(ours.state) == 0


def test_library_refuses_bad_arguments_on_the_host():
  from dynibar_amd import _lib
  lib = _lib.lib()
  assert lib.dyn_adam_step(None, None) == -1 and b'null params' in lib.dyn_last_error()
  q = _lib.params('DynAdamParams', n_tensors=1, n_chunks=1)
  assert lib.dyn_adam_step(q, None) == -1 and b'required' in lib.dyn_last_error()
  import ctypes
  buf = (ctypes.c_double * 16)()
  at = ctypes.addressof(buf)
  q = _lib.params('DynAdamParams', tensors=ctypes.c_void_p(at), chunks=ctypes.c_void_p(at), n_tensors=0, n_chunks=1)
  assert lib.dyn_adam_step(q, None) == -1 and b'0 tensors' in lib.dyn_last_error()
  q = _lib.params('DynAdamParams', tensors=ctypes.c_void_p(at + 4), chunks=ctypes.c_void_p(at), n_tensors=1, n_chunks=1)
  assert lib.dyn_adam_step(q, None) == -1 and b'8 bytes' in lib.dyn_last_error()
  names = [lib.dyn_profile_name(i).decode() for i in range(lib.dyn_profile_count())]
  assert names.count('k_adam_step') == 1
  for name in _lib.ENGINE_LIBS:
    assert hasattr(ctypes.CDLL(_lib.engine_path(name)), 'dyn_adam_step'), name
