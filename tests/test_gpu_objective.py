"""The training objective on the MI355X (dynibar_amd/objective.py, csrc/dyn_objective.h): every logged scalar and every cotangent against
the float64 restatement of train.py:300-456 (tests/objective_cases.py), exact zeros, bitwise reproducibility, eff_distloss_native on its
own, and end to end -- render_rays_mono(is_train=True) -> MonoObjective -> backward() -- against the real reference's autograd gradients
(tests/golden/mono_train_grad.npz, mono_train_grad_init.npz)."""
import pytest
import torch

import cases
import objective_cases as oc
import parity

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SINGLE = [(k, v) for k, v in cases.MONO_TRAIN_LOSSES.items() if k != 'full']


@pytest.mark.parametrize('R,S', [(37, 5), (3, 2), (257, 200), (3072, 64), (1024, 300)])
@pytest.mark.parametrize('epoch', oc.EPOCHS)
def test_objective_full(R, S, epoch):
  """every logged scalar and every cotangent against float64, the limit from the fp32 torch form's own error; 257 x 200 and 1024 x 300 walk
  the scan carry, 3072 x 64 is the training shape of configs/train_kid-running.txt"""
  oc.check_objective(DEV, R, S, epoch=epoch)


@pytest.mark.parametrize('nv', [1, 2, 3, 4, 5, 6])
def test_objective_flow_views(nv):
  oc.check_objective(DEV, 64, 64, nv=nv, epoch=0)


@pytest.mark.parametrize('name,terms', SINGLE, ids=[k for k, _ in SINGLE])
@pytest.mark.parametrize('epoch', oc.EPOCHS)
def test_objective_single_terms(name, terms, epoch):
  oc.check_objective(DEV, 37, 5, epoch=epoch, terms=terms)
  oc.check_objective(DEV, 3072, 64, epoch=epoch, terms=terms, seed=9)


def test_objective_anneal_cycle_off():
  oc.check_objective(DEV, 37, 5, epoch=2000, args=oc.args_of(anneal_cycle=False))


def test_exact_zeros_and_untouched_inputs():
  oc.check_exact_zeros(DEV)
  oc.check_exact_zeros(DEV, R=3072, S=64, seed=9)


@pytest.mark.parametrize('S', [2, 3, 63, 64, 65, 128, 129, 300])
def test_eff_distloss_native(S):
  oc.check_distloss(DEV, S)
  oc.check_distloss(DEV, S, R=1031)


def test_limits():
  from dynibar_amd import objective
  ret, tgt = oc.make_case(4, 1, nv=2, T=1)
  r, t, _ = oc.instantiate(ret, tgt, torch.float32, DEV)
  with pytest.raises(ValueError, match='at least 2 samples'):
    objective.MonoObjective(oc.args_of())(r, t, 0)
  ret, tgt = oc.make_case(4, 8, nv=7, T=1)
  r, t, _ = oc.instantiate(ret, tgt, torch.float32, DEV)
  with pytest.raises(ValueError, match='flow views'):
    objective.MonoObjective(oc.args_of())(r, t, 0)
  ret, tgt = oc.make_case(4, 8, nv=2, T=1)
  r, t, _ = oc.instantiate(ret, tgt, torch.float32, 'cpu')
  with pytest.raises(ValueError, match='HIP device'):
    objective.MonoObjective(oc.args_of())(r, t, 0)


def _train_step(terms, weights, trainable=None):
  """parity.run_mono_train_step with the product objective in place of the restated loss"""
  from dynibar_amd import objective, render_ray
  c = parity.MONO_TRAIN_CASE
  ret, model, fms = parity.mono_train_forward(DEV, c, weights, trainable)
  loss, logged = objective.MonoObjective(oc.args_of())(ret, cases.train_batch_targets(c['R']), 0, terms)
  loss.backward()
  grads = {'basis': model.trajectory_basis.grad}
  grads.update({leaf: fm.grad for leaf, fm in fms.items()})
  for net in ('net_coarse_st', 'net_coarse_dy', 'motion_mlp'):
    for k, p in render_ray._unwrap(getattr(model, net)).named_parameters():
      grads[f'{net}.{k}'] = p.grad
  return loss.detach(), logged, grads


@pytest.mark.parametrize('weights', ['trained', 'init'])
@pytest.mark.parametrize('lname', ['full', 'flow', 'cycle', 'reg', 'rgb'])
def test_end_to_end_against_the_reference(golden_dir, weights, lname):
  """render_rays_mono(is_train=True) -> MonoObjective -> backward(): the loss (1e-5 + 2e-4 relative, as parity.check_train_mono) and the
  gradient of every parameter, of the trajectory basis and of the feature maps against the REAL reference's autograd digests, with the weights
  of configs/train_kid-running.txt at epoch 0"""
  golden = cases.load_golden(golden_dir, 'mono_train_grad.npz' if weights == 'trained' else 'mono_train_grad_init.npz')
  loss, logged, grads = _train_step(cases.MONO_TRAIN_LOSSES[lname], weights)
  tag = f'objective end to end [{lname}] ({weights} weights)'
  print(f'  {tag}: loss {float(loss)!r} reference {float(golden[f"{lname}/loss"])!r} logged {logged.tolist()}')
  parity.assert_close(loss, torch.from_numpy(golden[f'{lname}/loss']), 1e-5, 2e-4, f'{tag} loss')
  keys = sorted({k.split('/')[1] for k in golden if k.startswith(lname + '/') and k.count('/') == 2})
  gmax = max(float(golden[f'{lname}/{k}/absmax'][0]) for k in keys if not k.startswith('featmaps'))
  n = 0
  for k in keys:
    ref_d = {dk: golden[f'{lname}/{k}/{dk}'] for dk in ('proj', 'absmax', 'head', 'l1')}
    g = grads.get(k)
    if g is None:
      assert float(ref_d['absmax'][0]) == 0.0, f'{tag}: no gradient for {k} but the reference has one (max {float(ref_d["absmax"][0]):.2e})'
      continue
    parity._digest_close(g, ref_d, f'{tag} grad {k}', g.numel(), gmax)
    n += 1
  missing = [k for k, g in grads.items() if g is not None and f'{lname}/{k}/proj' not in golden and float(g.abs().max()) > 0]
  assert not missing, f'{tag}: gradients the reference does not produce: {missing[:5]}'
  assert n > 0


def test_end_to_end_frozen_leaves_get_no_gradient(golden_dir):
  """only DynibarStatic trains, flow loss: its gradients against the reference's, every other leaf's .grad None"""
  golden = cases.load_golden(golden_dir, 'mono_train_grad_init.npz')
  loss, _, grads = _train_step(cases.MONO_TRAIN_LOSSES['flow'], 'init', trainable=parity.FREEZE_PATTERNS['st'])
  parity.assert_close(loss, torch.from_numpy(golden['flow/loss']), 1e-5, 2e-4, 'objective end to end frozen [flow] loss')
  keys = sorted({k.split('/')[1] for k in golden if k.startswith('flow/') and k.count('/') == 2})
  gmax = max(float(golden[f'flow/{k}/absmax'][0]) for k in keys if not k.startswith('featmaps'))
  n = 0
  for k, g in grads.items():
    if parity.leaf_of(k) != 'st':
      assert g is None, f'frozen leaf {k} received a gradient'
    elif g is not None and f'flow/{k}/proj' in golden:
      parity._digest_close(g, {dk: golden[f'flow/{k}/{dk}'] for dk in ('proj', 'absmax', 'head', 'l1')}, f'objective end to end frozen [flow] grad {k}',
                           g.numel(), gmax)
      n += 1
  assert n > 0


def test_no_synchronisation_in_forward_or_backward():
  """neither direction synchronises or reads a value back: torch's sync debug mode raises on any blocking call inside the region"""
  from dynibar_amd import objective
  ret, tgt = oc.make_case(512, 64)
  r, t, leaves = oc.instantiate(ret, tgt, torch.float32, DEV)
  obj = objective.MonoObjective(oc.args_of())
  loss, _ = obj(r, t, 2000)  # (first call: library load, allocator growth)
  loss.backward()
  torch.cuda.synchronize()
  torch.cuda.set_sync_debug_mode('error')
  try:
    loss, logged = obj(r, t, 2000)
    loss.backward()
  finally:
    torch.cuda.set_sync_debug_mode('default')
  assert len(logged.tolist()) == len(oc.LOGGED)
  # (at epoch 2000 the dynamic-only colour term is off: rgb_dy is the one leaf no term reaches)
  assert all((v.grad is not None) == (k != ('outputs_coarse_ref', 'rgb_dy')) for k, v in leaves.items())
