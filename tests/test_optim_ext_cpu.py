"""Host-side checks of the extended optimizer step (dynibar_amd/optim.py, csrc/dyn_optim.h): the yardstick itself -- the numpy restatement of
tests/optim_ext_cases.py against torch.optim.Adam / AdamW in float64, within twice torch's own fp32 distance --, the constructor, the record
layout, what is still refused, and state_dicts in both directions.  No kernel runs here; the kernels are compared with the restatement in
tests/emu/test_emu_optim_ext.py and tests/test_gpu_optim_ext.py."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_ext_cases as xc
from dynibar_amd import _lib, optim

F, D = np.float32, np.float64


def _restated(name, device_counts):
  cls, kw = xc.OPTION_SETS[name]
  p, grads = xc.torch_data(name)
  n = p.size
  m, v, vmax, pw = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F) if kw.get('amsgrad') else None, np.ones(2, D)
  lam, dec = kw.get('weight_decay', 0.0), cls == 'AdamW'
  for t, g in enumerate(grads[:xc.STEPS], 1):
    if device_counts:
      a, s2, pw = xc.pow_scalars(xc.LR_TORCH, 0.9, 0.999, pw)
    else:
      a, s2 = oc.scalars(xc.LR_TORCH, 0.9, 0.999, t)
    p, m, v, vmax = xc.restate(p, g, m, v, vmax, a, s2, 0.9, 0.999, 1e-8, wd=0.0 if dec else lam,
                               decay=xc.decay_factor(xc.LR_TORCH, lam) if dec else 1.0, maximize=bool(kw.get('maximize')))
  return p


@pytest.mark.parametrize('device_counts', (False, True))
@pytest.mark.parametrize('name', sorted(xc.OPTION_SETS))
def test_restatement_is_within_twice_torchs_fp32_distance_of_float64(name, device_counts):
  ref = xc.torch_reference(name)
  ours = float(np.abs(_restated(name, device_counts).astype(D) - ref['p64']).max())
  print(f'  {name}{" (device counts)" if device_counts else ""}: d = {ref["d"]:.3e}  restatement {ours:.3e}  ratio {ours / ref["d"]:.3f}')
  assert ref['d'] > 0 and ours <= 2 * ref['d']


def test_device_scalars_follow_the_hosts():
  """the running products beta^t of the device against torch's beta ** t: a and s2 agree to an fp32 ulp over a long run"""
  for lr, b1, b2 in ((4e-4, 0.9, 0.999), (1e-3, 0.85, 0.995)):
    pw = np.ones(2, D)
    for t in range(1, 3001):
      a, s2, pw = xc.pow_scalars(lr, b1, b2, pw)
      wa, ws2 = oc.scalars(lr, b1, b2, t)
      assert abs(float(a) - float(wa)) <= float(np.spacing(abs(wa))) and abs(float(s2) - float(ws2)) <= float(np.spacing(ws2)), (t, a, wa, s2, ws2)
  a, s2, _ = xc.pow_scalars(0.0, 0.9, 0.999, np.ones(2, D))
  assert a == 0 and np.signbit(a)  # lr = 0: -0.0, as the host forms it
  assert xc.decay_factor(1e-3, 1e-2) == F(1 - 1e-5) and xc.decay_factor(0.0, 0.1) == F(1)


def test_amsgrad_of_the_restatement_keeps_vmax_on_nan():
  one = np.ones(3, F)
  v0 = np.array([1.0, 4.0, 2.0], F)
  vmax0 = np.array([2.0, 3.0, 5.0], F)
  g = np.array([np.nan, 0.0, 0.0], F)
  _, _, v, vmax = xc.restate(one, g, 0 * one, v0, vmax0, -1e-3, 1.0, 0.9, 0.5, 1e-8)
  assert np.isnan(v[0]) and vmax[0] == 2.0 and vmax[1] == 3.0 and v[1] == 2.0 and vmax[2] == 5.0
  assert bool(torch.isnan(torch.maximum(torch.tensor(2.0), torch.tensor(float('nan')))))  # (where torch would store the NaN)


def test_record_layout_is_the_headers():
  X = optim.XRECORD
  assert X.itemsize == 128 and optim.RECORD.itemsize == 72
  assert [(k, X.fields[k][1]) for k in X.names] == [
      ('p', 0), ('g', 8), ('m', 16), ('v', 24), ('n', 32), ('a', 40), ('s2', 44), ('c1', 48), ('c2', 52), ('beta2', 56), ('eps', 60), ('skip', 64),
      ('flags', 68), ('vmax', 72), ('wd', 80), ('decay', 84), ('pow', 88), ('step', 96), ('lr_d', 104), ('beta1_d', 112), ('beta2_d', 120)]
  for k in optim.RECORD.names[:-1]:
    assert X.fields[k] == optim.RECORD.fields[k]


def test_library_refuses_bad_arguments_on_the_host():
  lib = _lib.lib()
  buf = (ctypes.c_double * 16)()
  at = ctypes.addressof(buf)
  ok = dict(tensors=ctypes.c_void_p(at), chunks=ctypes.c_void_p(at), n_tensors=1, n_chunks=1)
  for name, struct, more in (('dyn_adamx_step', 'DynAdamXParams', {}), ('dyn_adamx_step_guarded', 'DynAdamXGuardedParams', dict(stats=ctypes.c_void_p(at)))):
    fn = getattr(lib, name)
    assert fn(None, None) == -1 and b'null params' in lib.dyn_last_error() and name.encode() in lib.dyn_last_error()
    assert fn(_lib.params(struct, n_tensors=1, n_chunks=1, **more), None) == -1 and b'tensors and chunks are required' in lib.dyn_last_error()
    assert fn(_lib.params(struct, **dict(ok, n_tensors=0), **more), None) == -1 and b'0 tensors' in lib.dyn_last_error()
    assert fn(_lib.params(struct, **dict(ok, n_chunks=0), **more), None) == -1 and b'0 chunks' in lib.dyn_last_error()
    assert fn(_lib.params(struct, **dict(ok, tensors=ctypes.c_void_p(at + 4)), **more), None) == -1 and b'8 bytes' in lib.dyn_last_error()
  assert lib.dyn_adamx_step_guarded(_lib.params('DynAdamXGuardedParams', **ok), None) == -1 and b'stats is required' in lib.dyn_last_error()
  names = [lib.dyn_profile_name(i).decode() for i in range(lib.dyn_profile_count())]
  for kernel in ('k_adam_step', 'k_adam_step_guarded', 'k_adamx_step', 'k_adamx_step_guarded', 'k_adam_advance'):
    assert names.count(kernel) == 1, kernel
  for name in _lib.ENGINE_LIBS:
    flavour = ctypes.CDLL(_lib.engine_path(name))
    assert hasattr(flavour, 'dyn_adamx_step') and hasattr(flavour, 'dyn_adamx_step_guarded'), name


def _host_model(seed=0):
  g = torch.Generator().manual_seed(seed)
  return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((7, 3), (5,), (), (2, 3, 4))]


def test_constructors_are_torchs():
  from dynibar_amd.optim import AdamW
  ps = _host_model()
  from dynibar_amd.optim import AdamX
  for ours_cls, theirs_cls, kw in ((AdamX, torch.optim.Adam, dict(weight_decay=0.1, amsgrad=True, maximize=True, capturable=True)),
                                   (AdamX, torch.optim.Adam, dict(weight_decay=0.1, decoupled_weight_decay=True)), (AdamX, torch.optim.Adam, {}),
                                   (AdamW, torch.optim.AdamW, {}), (AdamW, torch.optim.AdamW, dict(weight_decay=0.3, amsgrad=True, maximize=True))):
    ours, theirs = ours_cls(ps, lr=2e-4, **kw), theirs_cls(ps, lr=2e-4, **kw)
    assert isinstance(ours, torch.optim.Optimizer) and ours.defaults == theirs.defaults
    assert ours.state_dict() == theirs.state_dict()
  assert AdamW(ps).defaults['weight_decay'] == 1e-2 and AdamW(ps).defaults['decoupled_weight_decay'] is True
  assert issubclass(AdamW, AdamX) and issubclass(optim.Adam, AdamX) and not issubclass(AdamW, optim.Adam)
  mixed = AdamX([dict(params=ps[:2], weight_decay=0.1), dict(params=ps[2:], amsgrad=True, maximize=True)], lr=1e-3)
  assert [g['weight_decay'] for g in mixed.param_groups] == [0.1, 0] and [g['amsgrad'] for g in mixed.param_groups] == [False, True]


def test_what_is_still_refused():
  for kw, match in ((dict(differentiable=True), 'differentiable'), (dict(foreach=False), 'foreach'), (dict(foreach=True), 'foreach'),
                    (dict(fused=False), 'fused'), (dict(fused=True), 'fused')):
    for cls in (optim.AdamX, optim.AdamW):
      with pytest.raises(NotImplementedError, match=match):
        cls(_host_model(), **kw)
  for cls in (optim.AdamX, optim.AdamW):
    with pytest.raises(ValueError, match='lr must be a number'):
      cls(_host_model(), lr=torch.tensor(1e-3))
    with pytest.raises(ValueError, match='weight_decay'):
      cls(_host_model(), weight_decay=-0.1)
  with pytest.raises(ValueError, match='weight_decay of group 0'):
    optim.AdamX([{'params': _host_model(), 'weight_decay': -1.0}])
  for kw, match in ((dict(amsgrad=True), 'AdamX has it'), (dict(weight_decay=0.1), 'AdamW')):  # optim.Adam itself is what it was, and says where to go
    with pytest.raises(NotImplementedError, match=match):
      optim.Adam(_host_model(), **kw)
  ours = optim.AdamX(_host_model(), amsgrad=True)
  ours.param_groups[0]['differentiable'] = True
  with pytest.raises(NotImplementedError, match=r'differentiable=True \(group 0\)'):
    ours.step()
  # host tensors are refused with the new options as with the old: there is no CPU fallback, nothing changes
  ps = _host_model()
  for p in ps:
    p.grad = torch.ones_like(p)
  before = [p.detach().clone() for p in ps]
  for kw in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True), dict(capturable=True)):
    ours = optim.AdamW(ps, **kw)
    with pytest.raises(RuntimeError, match='HIP device'):
      ours.step(skip_nonfinite=True)
    assert len(ours.state) == 0 and all(torch.equal(b, p.detach()) for b, p in zip(before, ps))
  sparse = torch.nn.Parameter(torch.ones(4, 3))
  sparse.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3))
  with pytest.raises(RuntimeError, match='sparse'):
    optim.AdamW([sparse]).step()


def _torch_steps(ps, opt, k, seed):
  g = torch.Generator().manual_seed(seed)
  for _ in range(k):
    for p in ps:
      p.grad = torch.randn(p.shape, generator=g)
    opt.step()


def _same_state(a, b):
  assert a['param_groups'] == b['param_groups'] and a['state'].keys() == b['state'].keys()
  for k in a['state']:
    assert a['state'][k].keys() == b['state'][k].keys(), (a['state'][k].keys(), b['state'][k].keys())
    for name in a['state'][k]:
      x, y = a['state'][k][name], b['state'][k][name]
      assert x.dtype == y.dtype and x.device == y.device and x.shape == y.shape and torch.equal(x, y), (k, name)


@pytest.mark.parametrize('cls,kw', [('Adam', dict(weight_decay=0.1, amsgrad=True)), ('AdamW', dict(amsgrad=True, maximize=True)), ('AdamW', {})])
def test_state_dict_goes_both_ways(cls, kw):
  ps = _host_model()
  theirs = getattr(torch.optim, cls)([dict(params=ps[:2], lr=4e-4), dict(params=ps[2:], betas=(0.8, 0.99))], lr=2e-4, **kw)
  _torch_steps(ps, theirs, 3, 1)
  sd = copy.deepcopy(theirs.state_dict())
  mine = [torch.nn.Parameter(p.detach().clone()) for p in ps]
  ours = xc.ours_class(cls)([dict(params=mine[:2]), dict(params=mine[2:])])
  ours.load_state_dict(copy.deepcopy(sd))
  _same_state(ours.state_dict(), sd)  # torch's keys and nothing else: max_exp_avg_sq where amsgrad, no beta_pow
  assert ours.param_groups[1]['betas'] == (0.8, 0.99) and ours.param_groups[0]['amsgrad'] == bool(kw.get('amsgrad'))
  assert ours.param_groups[0]['decoupled_weight_decay'] is (cls == 'AdamW')
  back = [torch.nn.Parameter(p.detach().clone()) for p in ps]
  again = getattr(torch.optim, cls)([dict(params=back[:2]), dict(params=back[2:])])
  again.load_state_dict(copy.deepcopy(ours.state_dict()))
  _torch_steps(ps, theirs, 2, 2)
  _torch_steps(back, again, 2, 2)
  assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(ps, back))


def test_capturable_checkpoints_on_the_host():
  """load_state_dict with capturable groups: beta_pow stays float64 bit for bit, a checkpoint without it gets [beta1 ** t, beta2 ** t], an
  integer step of an old checkpoint becomes torch's tensor, and torch loads what this class saves"""
  ps = _host_model()
  theirs = torch.optim.AdamW([dict(params=ps[:2]), dict(params=ps[2:], betas=(0.8, 0.99))], lr=2e-4, amsgrad=True)
  _torch_steps(ps, theirs, 3, 1)
  sd = copy.deepcopy(theirs.state_dict())
  for g in sd['param_groups']:
    g['capturable'] = True
  ours = optim.AdamW([dict(params=ps[:2]), dict(params=ps[2:])])
  ours.load_state_dict(copy.deepcopy(sd))
  for gi, (b1, b2) in enumerate(((0.9, 0.999), (0.8, 0.99))):
    for p in ours.param_groups[gi]['params']:
      st = ours.state[p]
      assert st['step'].dtype == torch.float32 and st['step'].dim() == 0 and float(st['step']) == 3.0
      assert st['beta_pow'].dtype == torch.float64 and st['beta_pow'].tolist() == [b1 ** 3.0, b2 ** 3.0]
  mine = copy.deepcopy(ours.state_dict())
  odd = torch.tensor([0.9 ** 3 * (1 + 2.0 ** -40), 0.999 ** 3 * (1 - 2.0 ** -45)], dtype=torch.float64)  # (no fp32 value: a cast would show)
  mine['state'][0]['beta_pow'] = odd.clone()
  again = optim.AdamW([dict(params=ps[:2]), dict(params=ps[2:])])
  again.load_state_dict(mine)
  assert again.state[ps[0]]['beta_pow'].dtype == torch.float64 and torch.equal(again.state[ps[0]]['beta_pow'], odd)
  assert again.state[ps[0]]['beta_pow'] is not mine['state'][0]['beta_pow']
  assert torch.equal(again.state_dict()['state'][0]['beta_pow'], odd)
  old = copy.deepcopy(sd)
  for st in old['state'].values():
    st['step'] = int(st['step'])
  older = optim.AdamW([dict(params=ps[:2]), dict(params=ps[2:])])
  older.load_state_dict(old)
  assert all(torch.is_tensor(older.state[p]['step']) and float(older.state[p]['step']) == 3.0 and 'beta_pow' in older.state[p] for p in ps)
  plain = copy.deepcopy(again.state_dict())
  for g in plain['param_groups']:
    g['capturable'] = False
  host = optim.AdamW([dict(params=ps[:2]), dict(params=ps[2:])])
  host.load_state_dict(plain)
  assert all('beta_pow' not in host.state[p] for p in ps)  # groups that are not capturable carry none
  back = [torch.nn.Parameter(p.detach().clone()) for p in ps]
  torchs = torch.optim.AdamW([dict(params=back[:2]), dict(params=back[2:])])
  torchs.load_state_dict(copy.deepcopy(again.state_dict()))  # beta_pow is an extra key torch carries along
  assert all(float(torchs.state[p]['step']) == 3.0 and torch.equal(torchs.state[p]['max_exp_avg_sq'], theirs.state[q]['max_exp_avg_sq'])
             for p, q in zip(back, ps))
