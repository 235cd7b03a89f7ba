"""The yardstick of the objective tests, without a device: the restatement of train.py:300-456 with its schedule (tests/objective_cases.py)
equals cases.mono_train_loss at epoch 0 (so it inherits that function's pin to the real reference, tests/golden/mono_train_grad*.npz), takes
every branch of the schedule, and cases._distloss equals the O(S^2) definition of the distortion loss.  These pass without the feature by design."""
import pytest
import torch

import cases
import objective_cases as oc


@pytest.mark.parametrize('terms', list(cases.MONO_TRAIN_LOSSES))
def test_restatement_equals_cases_loss_at_epoch_0(terms):
  ret, tgt = oc.make_case(37, 5, nv=6, seed=7)
  r, t, _ = oc.instantiate(ret, tgt, torch.float64, 'cpu')
  mine, _ = oc.mono_objective_loss(r, t, oc.args_of(), 0, cases.MONO_TRAIN_LOSSES[terms])
  theirs = cases.mono_train_loss(r, t, cases.MONO_TRAIN_LOSSES[terms], epoch=0)
  assert abs(float(mine) - float(theirs)) <= 1e-12 * abs(float(theirs)), (float(mine), float(theirs))


def test_generator_covers_every_branch():
  """3072 x 64, seed 7: rays below the 0.1 ratio threshold, rays below the depth clamp, no threshold ties, exact zeros on the tail, every term non-zero"""
  ret, tgt = oc.make_case(3072, 64, seed=7)
  ratio = oc.assert_no_ties(ret)
  assert 200 < int((ratio < 0.1).sum()) < 400
  assert 1 <= int((ret['outputs_coarse_ref']['depth'] < 1e-2).sum()) <= 12
  anc = ret['outputs_coarse_anchor']
  nt = oc.n_tail(64)
  assert nt == 6 and bool((anc['sf_seq'][:, :, -nt:] == 0).all()) and bool(((anc['pts_traj_ref'] - anc['pts_traj_anchor'])[:, :, -nt:] == 0).all())
  r, t, _ = oc.instantiate(ret, tgt, torch.float64, 'cpu')
  _, log = oc.mono_objective_loss(r, t, oc.args_of(), 2000)
  assert all(float(v) != 0.0 for v in log.values()), {k: float(v) for k, v in log.items()}


def test_schedule_branches():
  """divisor 0, 1, 5 with init_decay_epoch from the config; anneal_cycle on and off; the 0.5 cap reached"""
  ret, tgt = oc.make_case(64, 16, seed=8)
  r, t, _ = oc.instantiate(ret, tgt, torch.float64, 'cpu')
  log = {e: {k: float(v) for k, v in oc.mono_objective_loss(r, t, oc.args_of(), e)[1].items()} for e in oc.EPOCHS}
  assert log[400]['disp'] == pytest.approx(log[0]['disp'] / 10.0, rel=1e-12) and log[2000]['flow'] == pytest.approx(log[0]['flow'] / 1e5, rel=1e-12)
  assert log[400]['cycle'] == pytest.approx(2.0 * log[0]['cycle'], rel=1e-12)   # 0.1 + 1 * 0.1
  assert log[2000]['cycle'] == pytest.approx(5.0 * log[0]['cycle'], rel=1e-12)  # min(0.5, 0.1 + 5 * 0.1)
  off = float(oc.mono_objective_loss(r, t, oc.args_of(anneal_cycle=False), 2000)[1]['cycle'])
  assert off == pytest.approx(log[0]['cycle'], rel=1e-12)
  assert log[400]['rgb'] < log[0]['rgb']            # the dynamic-only term is gone, the _dy terms decayed
  assert log[2000]['static'] > log[400]['static']   # the divisor > 4 addition
  assert log[400]['static'] == pytest.approx(log[0]['static'], rel=1e-12) and log[400]['reg'] == log[0]['reg']


@pytest.mark.parametrize('S', [2, 33, 64])
def test_distloss_equals_the_quadratic_definition(S):
  g = torch.Generator().manual_seed(S)
  w = torch.rand(4, S, generator=g, dtype=torch.float64)
  edges = torch.sort(torch.rand(4, S + 1, generator=g, dtype=torch.float64), dim=-1).values
  m, d = (edges[:, 1:] + edges[:, :-1]) * 0.5, edges[:, 1:] - edges[:, :-1]
  a, b = float(cases._distloss(w, m, d)), float(oc.distloss_quadratic(w, m, d))
  assert abs(a - b) <= 1e-13 * abs(b), (a, b)
