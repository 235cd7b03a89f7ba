"""The extended optimizer step on the MI355X (dynibar_amd/optim.py, csrc/dyn_optim.h: k_adamx_step, k_adamx_step_guarded, k_adam_advance) against
the numpy restatement of tests/optim_ext_cases.py, exactly (torch.equal; NaNs by position), against torch.optim.Adam / AdamW within twice
torch's own fp32 noise, and the visibility of a fused step to the cached inference weights."""
import copy
import types

import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_ext_cases as xc
from dynibar_amd import optim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('guarded,zero_grads,capturable', xc.BITWISE_CASES)
def test_four_groups_in_one_launch_bitwise(guarded, zero_grads, capturable):
  xc.check_bitwise(DEV, guarded, zero_grads, capturable)


@pytest.mark.parametrize('shape', xc.SHAPES)
def test_every_option_on_one_tensor(shape):
  xc.check_single_float_path(DEV, shape)


@pytest.mark.parametrize('guarded', (False, True))
def test_old_path_unchanged(guarded):
  xc.check_old_path_unchanged(DEV, guarded)


def test_exact_skip():
  xc.check_exact_skip(DEV)


@pytest.mark.parametrize('name', sorted(xc.OPTION_SETS))
def test_against_torch_and_state_dicts_both_ways(name):
  xc.check_interop(DEV, name)


def test_capturable_state():
  xc.check_capturable_state(DEV)


def test_our_capturable_checkpoint_continues_in_torchs_capturable_adamw():
  """torch's capturable AdamW steps on the device only: it loads what ours saved (beta_pow is an extra key it ignores) and its next step
  stays within 2 d of ours"""
  name = 'adamw_amsgrad_maximize'
  cls, kw = xc.OPTION_SETS[name]
  ref = xc.torch_reference(name)
  q, opt, grads = xc.check_against_torch(DEV, name, capturable=True)
  tq = torch.nn.Parameter(q.detach().clone())
  theirs = torch.optim.AdamW([tq], lr=xc.LR_TORCH, capturable=True, **kw)
  theirs.load_state_dict(copy.deepcopy(opt.state_dict()))  # (a copy: torch's loader keeps tensors that need no cast, the two would share their moments)
  assert theirs.state[tq]['step'].is_cuda and float(theirs.state[tq]['step']) == xc.STEPS
  tq.grad = torch.from_numpy(grads[xc.STEPS].copy()).to(DEV)
  theirs.step()
  xc._step(q, opt, grads[xc.STEPS], DEV)
  dist = float((q.detach().double() - tq.detach().double()).abs().max())
  print(f'  ours capturable -> torch capturable AdamW, one further step: distance {dist:.3e} (2 d = {2 * ref["d"]:.3e})')
  assert dist <= 2 * ref['d'] and float(theirs.state[tq]['step']) == float(opt.state[q]['step']) == xc.STEPS + 1


def _launches(fn):
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


def test_launches_copies_and_allocations():
  """groups with different options share one launch; k_adam_advance runs only where a group is capturable; one host-to-device copy of both
  record tables, nothing back, no device memory after the first step; defaults still launch the plain kernels"""
  import test_gpu_scene as tgs
  for capturable in (False, True):
    groups, offsets = xc.mixed_groups(capturable)
    T = xc.Tensors(DEV, groups, seed=90, offsets=offsets)
    T.step(T.gradients())
    T.step(T.gradients(), max_grad_norm=1.0, skip_nonfinite=True)
    T.set_grads(T.gradients())
    torch.cuda.synchronize()
    advance = {'k_adam_advance': 1} if capturable else {}
    assert _launches(lambda: T.opt.step()) == dict({'k_adamx_step': 1}, **advance)
    assert _launches(lambda: T.opt.step(max_grad_norm=1.0, skip_nonfinite=True, zero_grads=True)) == dict(
        {'k_grad_sumsq': 1, 'k_grad_stats': 1, 'k_adamx_step_guarded': 1}, **advance)
    T.set_grads(T.gradients())
    torch.cuda.synchronize()
    allocations = torch.cuda.memory_stats(DEV)['allocation.all.allocated']  # (a count of allocations: what earlier tests free meanwhile does not move it)
    with tgs._Copies() as seen:
      T.opt.step()
      T.opt.step(max_grad_norm=1.0, skip_nonfinite=True)
    nbytes = len(T) * (optim.RECORD.itemsize + optim.XRECORD.itemsize)
    assert len(seen.h2d) == 2 and all(c[0].startswith('aten.copy_') and c[1] == [nbytes] for c in seen.h2d), seen.h2d
    assert seen.d2h == [], seen.d2h
    assert torch.cuda.memory_stats(DEV)['allocation.all.allocated'] == allocations
  P = oc.Tensors(DEV, [(dict(lr=4e-4), [4097, 3])], seed=91)
  P.set_grads(P.gradients())
  assert _launches(lambda: P.opt.step()) == {'k_adam_step': 1}
  assert _launches(lambda: P.opt.step(skip_nonfinite=True)) == {'k_grad_sumsq': 1, 'k_grad_stats': 1, 'k_adam_step_guarded': 1}


def _render(model, scene_args):
  from dynibar_amd import projection, render_ray
  fidx, temb, toff, batch, feat, args = scene_args
  with torch.no_grad():
    ret = render_ray.render_rays_mono((fidx, None), (temb.to(DEV), None), (toff, None), batch, model, feat, projection.Projector(DEV), 16, args,
                                      inv_uniform=True, det=True, is_train=False, num_vv=0)
  return {f'{grp}/{k}': v.detach().clone() for grp in ('outputs_coarse_ref', 'outputs_coarse_ref_dy', 'outputs_coarse_st')
          for k, v in ret[grp].items() if torch.is_tensor(v)}


@pytest.mark.parametrize('extended', (False, True))
def test_a_fused_step_is_visible_to_the_next_render(extended):
  """render, one fused step with a large lr, render again: the second render is, bit for bit, that of a fresh model object holding a copy
  of the updated weights (the packed inference weights were rebuilt), and it differs from the first"""
  import cases
  import parity
  scene, o, d, uv, _ = cases.scene_case('few')
  fidx, temb, toff = cases.time_args(scene['src_rgbs'].shape[1])
  args = types.SimpleNamespace(anti_alias_pooling=0, mask_rgb=1, input_dir=True, input_xyz=False, occ_weights_mode=0)
  scene_args = (fidx, temb, toff, parity.make_ray_batch(scene, o, d, uv, DEV),
                (scene['featmaps'].to(DEV), None, scene['static_featmaps'].to(DEV)), args)
  model = parity.make_module_model(DEV, args, wrap=False)
  names = ('net_coarse_st', 'net_coarse_dy', 'motion_mlp')
  params = [p for name in names for p in getattr(model, name).parameters()]
  first = _render(model, scene_args)
  gen = torch.Generator(device=DEV).manual_seed(7)
  for p in params:
    p.grad = torch.randn(p.shape, generator=gen, device=DEV)
  opt = optim.AdamX(params, lr=2e-2, amsgrad=True) if extended else optim.Adam(params, lr=2e-2)
  versions = [p._version for p in params]
  opt.step()
  second = _render(model, scene_args)
  weights = {name: {k: v.detach().cpu().numpy().copy() for k, v in getattr(model, name).state_dict().items()} for name in names}
  fresh = parity.make_module_model(DEV, args, wrap=False, weights=weights)
  with torch.no_grad():
    fresh.trajectory_basis.copy_(model.trajectory_basis)
  want = _render(fresh, scene_args)
  assert second.keys() == want.keys() and len(want) > 0
  differs = False
  for k in want:
    assert torch.equal(torch.nan_to_num(second[k].float()), torch.nan_to_num(want[k].float())), f'{k}: the render after the step is not the render of the updated weights'
    differs = differs or not torch.equal(second[k], first[k])
  assert differs, 'the step changed no output: the test shows nothing'
  assert all(p._version > v for p, v in zip(params, versions))  # (how the packed weights came to be rebuilt)
