"""The objective kernels (csrc/dyn_objective.h) under the wave-level emulator: the same checks as tests/test_gpu_objective.py through
objective_cases.check_objective, at the shapes a CPU can afford.  Debugging aid in a container without a GPU; -m gpu is authoritative."""
import pytest

import cases
import objective_cases as oc

pytestmark = pytest.mark.emu
TERMS = [('full', oc.ALL)] + [(k, v) for k, v in cases.MONO_TRAIN_LOSSES.items() if k != 'full']


@pytest.mark.parametrize('R,S', [(37, 5), (3, 2), (257, 200)])
@pytest.mark.parametrize('epoch', oc.EPOCHS)
def test_objective_full(emu, R, S, epoch):
  """every logged scalar and every cotangent against float64; 257 x 200 walks the scan carry over four chunks"""
  oc.check_objective(emu, R, S, epoch=epoch)


@pytest.mark.parametrize('nv', [1, 2, 3, 4, 5, 6])
def test_objective_flow_views(emu, nv):
  oc.check_objective(emu, 64, 64, nv=nv, epoch=0)


@pytest.mark.parametrize('name,terms', TERMS[1:], ids=[k for k, _ in TERMS[1:]])
@pytest.mark.parametrize('epoch', oc.EPOCHS)
def test_objective_single_terms(emu, name, terms, epoch):
  oc.check_objective(emu, 37, 5, epoch=epoch, terms=terms)


def test_objective_anneal_cycle_off(emu):
  oc.check_objective(emu, 37, 5, epoch=2000, args=oc.args_of(anneal_cycle=False))


def test_exact_zeros_and_untouched_inputs(emu):
  oc.check_exact_zeros(emu)


@pytest.mark.parametrize('S', [2, 3, 63, 64, 65, 128, 129, 300])
def test_eff_distloss_native(emu, S):
  oc.check_distloss(emu, S)


def test_schedule_weights():
  """MonoObjective.schedule: the weights handed to the kernels at the epochs that take every branch (no kernel runs)"""
  from dynibar_amd import objective
  sch = objective.MonoObjective(oc.args_of()).schedule
  assert sch(0)['k_rgb_dyn'] == 1.0 and sch(400)['k_rgb_dyn'] == 0.0 and sch(400)['k_rgb_dy'] == 0.1 and sch(2000)['w_cycle'] == 0.5
  assert sch(400)['w_disp'] == 0.1 / 10 and sch(2000)['w_flow'] == 0.01 / 10 ** 5 and sch(400)['w_cycle'] == 0.2
  assert sch(1999)['k_static2'] == 0.0 and sch(2000)['k_static2'] == 0.1 and sch(2000, ('flow',))['k_static2'] == 0.0
  assert objective.MonoObjective(oc.args_of(anneal_cycle=False)).schedule(2000)['w_cycle'] == 0.1
  with pytest.raises(ValueError, match='unknown terms'):
    sch(0, ('colour',))


def test_limits(emu):
  from dynibar_amd import objective
  import torch
  ret, tgt = oc.make_case(4, 1, nv=2, T=1)
  r, t, _ = oc.instantiate(ret, tgt, torch.float32, emu)
  with pytest.raises(ValueError, match='at least 2 samples'):
    objective.MonoObjective(oc.args_of())(r, t, 0)
  ret, tgt = oc.make_case(4, 8, nv=7, T=1)
  r, t, _ = oc.instantiate(ret, tgt, torch.float32, emu)
  with pytest.raises(ValueError, match='flow views'):
    objective.MonoObjective(oc.args_of())(r, t, 0)
  ret, tgt = oc.make_case(4, 8, nv=2, T=1)
  r, t, _ = oc.instantiate(ret, tgt, torch.float32, emu)
  r['outputs_coarse_anchor']['occ_weights'].requires_grad_(True)
  with pytest.raises(ValueError, match='carries a graph'):
    objective.MonoObjective(oc.args_of())(r, t, 0)
  r, t, _ = oc.instantiate(ret, tgt, torch.float64, emu)
  with pytest.raises(ValueError, match='float32'):
    objective.MonoObjective(oc.args_of())(r, t, 0)
