"""Host-side checks of the optimizer's guard (dynibar_amd/optim.py, csrc/dyn_optim.h): the yardstick itself -- the numpy restatement of the
norm / clip contract (tests/optim_guard_cases.py) against the float64 norm and torch.nn.utils.clip_grad_norm_ in float64 -- and every refusal
that needs no launch.  No kernel runs here; the kernels are compared with the restatement in tests/emu/test_emu_optim_guard.py and
tests/test_gpu_optim_guard.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

import optim_guard_cases as gc
from dynibar_amd import _lib, optim

F = np.float32


def _parameter_set(seed):
  """40 tensors of 1 .. 30 000 elements, each a standard normal times its own magnitude 10^k, k from -20 .. 15"""
  rng = np.random.default_rng([seed, 40])
  return [(rng.standard_normal(int(n)) * 10.0 ** rng.integers(-20, 16)).astype(np.float32) for n in rng.integers(1, 30001, 40)]


@pytest.fixture(scope='module')
def sets():
  out = []
  for seed in range(6):
    grads = _parameter_set(seed)
    partials, st = gc.restate_norm(grads, optim.CHUNK)
    out.append((grads, partials, st))
  return out


def test_restated_norm_is_within_one_ulp_of_the_float64_norm(sets):
  """the double sums of the contract lose far less than one fp32 ulp at these sizes; the final rounding to fp32 gives the rest"""
  for grads, _, st in sets:
    exact = math.sqrt(math.fsum(np.concatenate([g.astype(np.float64) * g.astype(np.float64) for g in grads])))  # (the squares are exact)
    ulp = float(np.spacing(F(exact)))
    print(f'  norm {float(st["norm"]):.9g}  float64 {exact:.17g}  distance {abs(float(st["norm"]) - exact) / ulp:.3f} ulp')
    assert st['finite'] == 1 and abs(float(st['norm']) - exact) <= ulp
    assert abs(float(st['sumsq']) - exact * exact) <= 1e-12 * exact * exact


def test_restated_clip_follows_torchs_in_float64(sets):
  """|g' - g64'| <= 2^-21 |g64'| + one fp32 subnormal: the norm is off by 2^-23 at most (one ulp), the addition of 1e-6, the division and
  the product by 2^-24 each -- 5 * 2^-24, rounded up"""
  for grads, partials, st in sets:
    max_norm = 0.37 * float(st['norm'])
    want = gc.finish(partials, max_norm)
    assert want['coef'] < 1
    ps = [torch.nn.Parameter(torch.zeros(g.size, dtype=torch.float64)) for g in grads]
    for p, g in zip(ps, grads):
      p.grad = torch.from_numpy(g).double()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    assert abs(float(total) - float(st['norm'])) <= float(np.spacing(st['norm']))
    worst = 0.0
    for p, g in zip(ps, grads):
      mine, ref = gc.scaled(g, want['coef']).astype(np.float64), p.grad.numpy()
      bound = 2.0 ** -21 * np.abs(ref) + 2.0 ** -149
      assert bool((np.abs(mine - ref) <= bound).all())
      nz = ref != 0
      worst = max(worst, float((np.abs(mine - ref)[nz] / np.abs(ref)[nz]).max()) if nz.any() else 0.0)
    print(f'  max_norm {max_norm:.4g}: coef {float(want["coef"]):.9g}, worst relative distance {worst / 2.0 ** -24:.3f} x 2^-24')


def test_coef_is_exactly_one_below_max_norm(sets):
  for grads, partials, st in sets:
    norm = float(st['norm'])
    for max_norm in (1.001 * norm + 2e-6, 2.0 * norm + 1.0, 1e30):
      assert gc.finish(partials, max_norm)['coef'] == F(1.0)
    assert gc.finish(partials, None)['coef'] == F(1.0) and gc.finish(partials, 0.0)['coef'] == F(1.0)
    assert gc.finish(partials, 0.999 * norm)['coef'] < F(1.0)
  nan = gc.finish(np.array([1.0, np.nan]), 1.0)
  assert nan['finite'] == 0 and nan['coef'] == F(1.0) and np.isnan(nan['norm'])
  inf = gc.finish(np.array([9e76, 9e76]), 1.0)  # two elements of 3e38
  assert inf['finite'] == 1 and np.isinf(inf['norm']) and inf['coef'] == F(0.0)


def test_lane_assignment_of_the_restatement():
  """element e of a chunk adds into lane (e >> 2) & 255: a chunk with one non-zero element per lane pair gives the butterfly's sum"""
  g = np.zeros(optim.CHUNK + 3, np.float32)
  g[[0, 4, 1024, optim.CHUNK - 1, optim.CHUNK + 2]] = [1.0, 2.0, 3.0, 4.0, 5.0]
  parts = gc.chunk_sums(g, optim.CHUNK)
  assert parts.shape == (2,) and parts[0] == 1.0 + 4.0 + 9.0 + 16.0 and parts[1] == 25.0
  assert gc.chunk_sums(np.zeros((), np.float32), optim.CHUNK).shape == (1,)


def test_stats_layout_is_the_headers():
  assert optim.STATS.names == ('sumsq', 'norm', 'coef', 'finite', 'reserved', 'calls', 'nonfinite') and optim.STATS.itemsize == 40
  assert [optim.STATS.fields[k][1] for k in optim.STATS.names] == [0, 8, 12, 16, 20, 24, 32]
  assert optim.GradStats._fields[:5] == ('norm', 'coef', 'finite', 'calls', 'nonfinite')


def test_library_refuses_bad_arguments_on_the_host():
  lib = _lib.lib()
  buf = (ctypes.c_double * 16)()
  at = ctypes.addressof(buf)
  ok = dict(tensors=ctypes.c_void_p(at), chunks=ctypes.c_void_p(at), n_tensors=1, n_chunks=1)
  extra = {'dyn_grad_norm': ('DynGradNormParams', dict(partials=ctypes.c_void_p(at), stats=ctypes.c_void_p(at))),
           'dyn_grad_scale': ('DynGradScaleParams', dict(stats=ctypes.c_void_p(at))),
           'dyn_adam_step_guarded': ('DynAdamGuardedParams', dict(stats=ctypes.c_void_p(at)))}
  for name, (struct, more) in extra.items():
    fn = getattr(lib, name)
    assert fn(None, None) == -1 and b'null params' in lib.dyn_last_error() and name.encode() in lib.dyn_last_error()
    assert fn(_lib.params(struct, n_tensors=1, n_chunks=1, **more), None) == -1 and b'tensors and chunks are required' in lib.dyn_last_error()
    assert fn(_lib.params(struct, **dict(ok, n_tensors=0), **more), None) == -1 and b'0 tensors' in lib.dyn_last_error()
    assert fn(_lib.params(struct, **dict(ok, n_chunks=0), **more), None) == -1 and b'0 chunks' in lib.dyn_last_error()
    assert fn(_lib.params(struct, **dict(ok, tensors=ctypes.c_void_p(at + 4)), **more), None) == -1 and b'8 bytes' in lib.dyn_last_error()
    assert fn(_lib.params(struct, **ok), None) == -1 and b'required' in lib.dyn_last_error() and b'stats' in lib.dyn_last_error()
    assert fn(_lib.params(struct, **ok, **dict(more, stats=ctypes.c_void_p(at + 4))), None) == -1 and b'8 bytes' in lib.dyn_last_error()
  q = _lib.params('DynGradNormParams', stats=ctypes.c_void_p(at), **ok)
  assert lib.dyn_grad_norm(q, None) == -1 and b'partials and stats are required' in lib.dyn_last_error()
  q = _lib.params('DynGradNormParams', stats=ctypes.c_void_p(at), partials=ctypes.c_void_p(at + 4), **ok)
  assert lib.dyn_grad_norm(q, None) == -1 and b'8 bytes' in lib.dyn_last_error()
  q = _lib.params('DynGradNormParams', stats=ctypes.c_void_p(at), partials=ctypes.c_void_p(at), max_norm=float('nan'), **ok)
  assert lib.dyn_grad_norm(q, None) == -1 and b'NaN' in lib.dyn_last_error()
  names = [lib.dyn_profile_name(i).decode() for i in range(lib.dyn_profile_count())]
  for kernel in ('k_adam_step', 'k_adam_step_guarded', 'k_grad_sumsq', 'k_grad_stats', 'k_grad_scale'):
    assert names.count(kernel) == 1, kernel
  assert lib.dyn_abi_version() == 1
  for name in _lib.ENGINE_LIBS:
    flavour = ctypes.CDLL(_lib.engine_path(name))
    for symbol in extra:
      assert hasattr(flavour, symbol), (name, symbol)


def _host_model():
  g = torch.Generator().manual_seed(0)
  ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((7, 3), (5,), ())]
  for p in ps:
    p.grad = torch.ones_like(p)
  return ps


def test_python_refuses_a_bad_max_grad_norm():
  ps = _host_model()
  opt = optim.Adam(ps, lr=1e-2)
  before = [p.detach().clone() for p in ps]
  for bad in (0, 0.0, -1.0, float('nan'), float('inf')):
    with pytest.raises(ValueError, match='finite number above 0'):
      opt.step(max_grad_norm=bad)
    with pytest.raises(ValueError, match='finite number above 0'):
      optim.clip_grad_norm_(ps, bad)
  with pytest.raises(ValueError, match='tensor max_grad_norm is not built'):
    opt.step(max_grad_norm=torch.tensor(1.0))
  assert opt.grad_stats is None and len(opt.state) == 0 and all(torch.equal(b, p.detach()) for b, p in zip(before, ps))


def test_python_refuses_other_norms_and_foreach():
  ps = _host_model()
  for norm_type in (1, 1.0, float('inf'), 3.0):
    with pytest.raises(NotImplementedError, match='norm_type'):
      optim.clip_grad_norm_(ps, 1.0, norm_type=norm_type)
  for foreach in (True, False):
    with pytest.raises(NotImplementedError, match='foreach'):
      optim.clip_grad_norm_(ps, 1.0, foreach=foreach)


def test_host_tensors_are_refused():
  """there is no CPU fallback for the guard either: nothing changes"""
  ps = _host_model()
  opt = optim.Adam(ps, lr=1e-2)
  before = [p.detach().clone() for p in ps]
  with pytest.raises(RuntimeError, match='HIP device'):
    opt.step(max_grad_norm=1.0, skip_nonfinite=True)
  for fn in (optim.grad_norm, lambda x: optim.clip_grad_norm_(x, 1.0)):
    with pytest.raises(RuntimeError, match='HIP device'):
      fn(ps)
  assert opt.grad_stats is None and len(opt.state) == 0
  assert all(torch.equal(b, p.detach()) for b, p in zip(before, ps)) and all(bool((p.grad == 1).all()) for p in ps)
  assert float(optim.grad_norm([])) == 0.0 and float(optim.clip_grad_norm_([torch.nn.Parameter(torch.zeros(3))], 1.0)) == 0.0
