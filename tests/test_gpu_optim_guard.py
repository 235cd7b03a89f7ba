"""The guard of the optimizer step on the MI355X (dynibar_amd/optim.py, csrc/dyn_optim.h: k_grad_sumsq, k_grad_stats, k_adam_step_guarded,
k_grad_scale) against the numpy restatement of tests/optim_guard_cases.py (itself held to the float64 norm and to torch's clip_grad_norm_:
tests/test_optim_guard_cpu.py).  Every comparison is exact (torch.equal; NaNs by position).  NaN and Inf gradients are data here."""
import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_guard_cases as gc
from dynibar_amd import optim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = gc.sizes(optim.CHUNK)
GUARD_KERNELS = {'k_grad_sumsq': 1, 'k_grad_stats': 1, 'k_adam_step_guarded': 1}


@pytest.mark.parametrize('shape', SIZES)
def test_single_tensor(shape):
  gc.check_single(DEV, shape)


@pytest.mark.parametrize('shape', SIZES)
def test_misaligned_views_sum_like_aligned_ones(shape):
  gc.check_misaligned(DEV, shape)


def test_600_tensors_from_nan_partials():
  gc.check_many(DEV, optim.CHUNK)


@pytest.mark.parametrize('kind', gc.VALUE_CASES)
def test_gradient_values(kind):
  gc.check_values(DEV, optim.CHUNK, kind)


@pytest.mark.parametrize('value,mode', gc.NONFINITE_CASES)
def test_injected_nonfinite(value, mode):
  gc.check_nonfinite(DEV, optim.CHUNK, value, mode)


def test_ten_guarded_steps_with_steplr_and_torchs_state():
  gc.check_steplr(DEV, optim.CHUNK)


def test_grad_norm_and_clip_on_their_own():
  gc.check_standalone(DEV, optim.CHUNK)


def _warm():
  T = oc.Tensors(DEV, oc.many_groups(optim.CHUNK), seed=27)
  T.set_grads(T.gradients())
  T.opt.step(max_grad_norm=1.0, skip_nonfinite=True)  # (the tables and the guard's buffers are made by the first step)
  T.set_grads(T.gradients())
  torch.cuda.synchronize()
  return T


def _launches(fn):
  """the library's kernels launched by fn(), by its own per-kernel counters"""
  from dynibar_amd import _lib
  lib = _lib.lib()
  n = lib.dyn_profile_count()
  ms, cnt = np.zeros(n, np.float32), np.zeros(n, np.int32)
  lib.dyn_profile_enable(1)
  try:
    lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
    fn()
    torch.cuda.synchronize()
    lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
  finally:
    lib.dyn_profile_enable(0)
  return {lib.dyn_profile_name(i).decode(): int(c) for i, c in enumerate(cnt) if c}


def test_a_guarded_step_is_three_launches():
  T = _warm()
  assert _launches(lambda: T.opt.step(max_grad_norm=1.0, skip_nonfinite=True)) == GUARD_KERNELS
  assert _launches(lambda: T.opt.step(skip_nonfinite=True, zero_grads=True)) == GUARD_KERNELS
  assert int(T.opt.grad_stats.calls) == 3


def test_a_guarded_step_copies_once_to_the_device_and_nothing_back():
  import test_gpu_scene as tgs
  T = _warm()
  allocated = torch.cuda.memory_allocated(DEV)
  with tgs._Copies() as seen:
    T.opt.step(max_grad_norm=1.0, skip_nonfinite=True)
    T.opt.step(max_grad_norm=0.5, zero_grads=True)
    stats = T.opt.grad_stats
  print('  two guarded steps: host-to-device', seen.h2d, 'device-to-host', seen.d2h)
  assert len(seen.h2d) == 2 and all(c[0].startswith('aten.copy_') and c[1] == [600 * optim.RECORD.itemsize] for c in seen.h2d), seen.h2d
  assert seen.d2h == [], seen.d2h
  assert torch.cuda.memory_allocated(DEV) == allocated  # no device memory after the first guarded step
  assert all(buf.is_pinned() for buf, _ in T.opt._staging)
  assert int(stats.calls) == 3 and int(stats.nonfinite) == 0 and float(stats.coef) < 1


def test_guarded_and_unguarded_steps_alternate():
  """an unguarded step() after a guarded one is the one k_adam_step launch it always was, on the same tables"""
  T = _warm()
  tables = T.opt._tables
  assert _launches(lambda: T.opt.step()) == {'k_adam_step': 1}
  assert _launches(lambda: T.opt.step(max_grad_norm=1.0)) == GUARD_KERNELS
  assert _launches(lambda: T.opt.step(zero_grads=True)) == {'k_adam_step': 1}
  assert T.opt._tables is tables and int(T.opt.grad_stats.calls) == 2


def test_training_loop_with_the_guarded_step_reduces_the_loss():
  import os
  import sys
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
  import train_loop
  h = train_loop.run(DEV, iters=6, R=64, log_every=5, quiet=True, optimizer='hip', max_grad_norm=1.0, skip_nonfinite=True)
  for stage in ('bootstrap', 'main'):
    print(f'  {stage}: {h[stage]}')
    assert np.isfinite(h[stage]).all() and h[stage][-1] < h[stage][0], (stage, h[stage])
  print('  grad_stats:', h['grad_stats'])
  assert h['grad_stats']['nonfinite'] == 0 and h['grad_stats']['finite'] == 1
  assert h['grad_stats']['calls'] == 12  # six guarded steps in each of the two stages
