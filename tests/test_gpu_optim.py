"""The optimizer on the MI355X (dynibar_amd/optim.py, csrc/dyn_optim.h) against the numpy restatement of tests/optim_cases.py (itself held to
torch.optim.Adam in float64: tests/test_optim_cpu.py).  Every comparison is exact (torch.equal; NaNs by position)."""
import numpy as np
import pytest
import torch

import optim_cases as oc
from dynibar_amd import optim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = oc.sizes(optim.CHUNK)


@pytest.mark.parametrize('shape', SIZES)
def test_single_tensor(shape):
  oc.check_single(DEV, shape)


@pytest.mark.parametrize('shape', SIZES)
def test_misaligned_views(shape):
  oc.check_misaligned(DEV, shape)


def test_600_tensors_in_6_groups():
  oc.check_many(DEV, optim.CHUNK)


def test_grad_none_between_two_updated():
  oc.check_grad_none_between(DEV, optim.CHUNK)


def test_first_gradient_at_step_4():
  oc.check_late_first_gradient(DEV, optim.CHUNK)


def test_lr_zero_group():
  oc.check_lr_zero(DEV)


@pytest.mark.parametrize('kind', oc.VALUE_CASES)
def test_gradient_values(kind):
  oc.check_values(DEV, optim.CHUNK, kind)


def test_ten_steps_with_steplr():
  oc.check_steplr(DEV, optim.CHUNK)


def test_continues_from_torchs_state():
  oc.check_loaded_state(DEV, optim.CHUNK)


def test_zero_grads():
  oc.check_zero_grads(DEV, optim.CHUNK)


def _warm():
  T = oc.Tensors(DEV, oc.many_groups(optim.CHUNK), seed=12)
  T.step(T.gradients())  # (the chunk list is uploaded and the moments are allocated by the first step)
  T.set_grads(T.gradients())
  torch.cuda.synchronize()
  return T


def test_a_step_is_one_launch():
  """the kernels of a step() over 600 tensors by the library's own per-kernel counters"""
  from dynibar_amd import _lib
  T = _warm()
  lib = _lib.lib()
  n = lib.dyn_profile_count()
  ms, cnt = np.zeros(n, np.float32), np.zeros(n, np.int32)
  lib.dyn_profile_enable(1)
  try:
    lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
    T.opt.step()
    torch.cuda.synchronize()
    lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
  finally:
    lib.dyn_profile_enable(0)
  launched = {lib.dyn_profile_name(i).decode(): int(c) for i, c in enumerate(cnt) if c}
  assert launched == {'k_adam_step': 1}, launched


def test_a_step_copies_once_to_the_device_and_nothing_back():
  import test_gpu_scene as tgs
  T = _warm()
  allocated = torch.cuda.memory_allocated(DEV)
  with tgs._Copies() as seen:
    T.opt.step()
    T.opt.step(zero_grads=True)
  print('  two steps: host-to-device', seen.h2d, 'device-to-host', seen.d2h)
  assert len(seen.h2d) == 2 and all(c[0].startswith('aten.copy_') and c[1] == [600 * optim.RECORD.itemsize] for c in seen.h2d), seen.h2d
  assert seen.d2h == [], seen.d2h
  assert torch.cuda.memory_allocated(DEV) == allocated  # no device memory after the first step
  assert all(buf.is_pinned() for buf, _ in T.opt._staging)


def test_device_refusals():
  oc.check_tensor_refusals(DEV)
  good = torch.nn.Parameter(torch.ones(6, device=DEV))
  host = torch.nn.Parameter(torch.ones(6))
  good.grad, host.grad = torch.ones(6, device=DEV), torch.ones(6)
  opt = optim.Adam([good, host], lr=1e-2)
  with pytest.raises(RuntimeError, match='HIP device'):
    opt.step()
  assert torch.equal(good.detach().cpu(), torch.ones(6)) and len(opt.state) == 0
  if torch.cuda.device_count() > 1:
    other = torch.nn.Parameter(torch.ones(6, device='cuda:1'))
    other.grad = torch.ones(6, device='cuda:1')
    with pytest.raises(RuntimeError, match='more than one device'):
      optim.Adam([good, other], lr=1e-2).step()


def test_training_loop_with_the_hip_optimizer_reduces_the_loss():
  """both stages of tools/train_loop.py with optimizer='hip': the bootstrap stage leaves the dynamic branch, the motion MLP and the basis
  without gradients (skipped records), the main stage updates everything"""
  import os
  import sys
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
  import train_loop
  h = train_loop.run(DEV, iters=6, R=64, log_every=5, quiet=True, optimizer='hip')
  for stage in ('bootstrap', 'main'):
    print(f'  {stage}: {h[stage]}')
    assert np.isfinite(h[stage]).all() and h[stage][-1] < h[stage][0], (stage, h[stage])
