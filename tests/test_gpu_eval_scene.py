"""The benchmark evaluation from a device-resident scene on the MI355X (dynibar_amd/scene.py for_evaluation ..., dynibar_amd/nvidia_eval.py,
csrc/dyn_eval.h) against the existing host path: ``scene.eval_sampler(step, view_plan).get_all()`` and
``RaySamplerSingleImage(data, dev).get_all()`` on the collated item that tests/eval_scene_cases.py restates from the same arrays
(eval_nvidia.py:71-198) give the same keys, shapes, dtypes and bits; every output element is written (the outputs start as NaN under the
suite: DYNIBAR_TRAIN_POISON, tests/conftest.py); the masked static views are the script's product bit for bit; a step's tensors and feature
maps are reused for its cameras without a change of bits, on any stream; a step costs one host-to-device copy, a view one more, a step one
device-to-host copy, and the loop adds no synchronising call to those of the renders themselves (the renderer, untouched here, reads the
image size back per projection context: 94 synchronising calls per 16 x 20 step with and without the loop, measured on an MI355X); the
mask pair equals numpy; both entry points refuse bad
arguments untouched; and one time step goes through ``nvidia_eval`` to exactly the numbers ``nvidia_frame_metrics`` gives on the host path's
frames.  Shapes: (5, 7) and (17, 19) make H*W*3 and H*W no multiples of 4 (scalar tails, views that do not start on 16 bytes), (16, 16) and
(18, 32) take the float4 stores.  All of these are less than one tile of 1024 pixels per view, so (40, 67) is added: three tiles per view,
more than one workgroup along x, with both tails."""
import types
import warnings

import numpy as np
import pytest
import torch

import eval_scene_cases as ec
import scene_cases as sc
from test_gpu_bullet import _Copies

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(16, 16), (17, 19), (5, 7), (18, 32)]


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('mask_static', [False, True])
@pytest.mark.parametrize('N', [12, 14])
def test_get_all_equals_the_host_sampler(H, W, mask_static, N):
  """render_idx 3 and N - 4, cameras 0 and 11; N = 14 at render_idx 3 selects static ids below 3 and at or above N - 3: masks exactly 1.0"""
  from dynibar_amd.train_static import POISON_SCRATCH
  assert POISON_SCRATCH
  ec.check_get_all(DEV, H, W, N, mask_static)


def test_get_all_with_double_bounds_and_many_tiles():
  """float64 bounds give a float64 depth_range like the reference's item; 40 x 67 takes three tiles of 1024 pixels per view"""
  ec.check_get_all(DEV, 40, 67, 14, True, bounds_dtype=np.float64)


def _model(seed=0):
  import cases
  from dynibar_amd import feature_network, synthetic as syn
  from test_gpu_bullet import _dct_basis
  enc = lambda s: feature_network.ResNet.from_module({k: torch.from_numpy(v).to(DEV) for k, v in syn.make_encoder_weights(s).items()})
  basis = _dct_basis(cases.NUM_BASIS, cases.NUM_FRAMES).to(DEV)
  return types.SimpleNamespace(net_coarse_st=syn.make_weights('static', 0), net_coarse_dy=syn.make_weights('dynamic', 0),
                               net_fine_st=syn.make_weights('static', 100), net_fine_dy=syn.make_weights('dynamic', 100),
                               motion_mlp=syn.make_weights('motion', 0, num_basis=cases.NUM_BASIS),
                               motion_mlp_fine=syn.make_weights('motion', 100, num_basis=cases.NUM_BASIS), trajectory_basis=basis,
                               trajectory_basis_fine=basis, feature_net=enc(0), feature_net_fine=enc(1))


def _step_bits(scene, model, render_idx, args, cam):
  """a fresh step plan, its tensors, the four feature maps and the view's get_all -> list of (name, tensor)"""
  from dynibar_amd import nvidia_eval
  plan = scene.eval_step_plan(render_idx, args)
  step = scene.assemble_eval_step(plan)
  with torch.no_grad():
    coarse, fine = nvidia_eval.encode_step(model, step)
  got = scene.eval_sampler(step, scene.eval_view_plan(plan, cam)).get_all()
  named = [(k, v) for k, v in sorted(got.items()) if isinstance(v, torch.Tensor)]
  named += [('masked', step.static_src_rgbs_masked), ('ref_time', step.ref_time), ('coarse ref', coarse[0]), ('coarse static', coarse[2]),
            ('fine ref', fine[0]), ('fine static', fine[2])]
  return step, (coarse, fine), named


def _assert_same_bits(got, want, what):
  assert [k for k, _ in got] == [k for k, _ in want]
  for (k, g), (_, w) in zip(got, want):
    assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), f'{what}: {k}'
    assert torch.equal(g.contiguous().view(torch.uint8).cpu(), w.contiguous().view(torch.uint8).cpu()), f'{what}: {k} differs'


def test_a_steps_tensors_are_reused_without_a_change_of_bits():
  """the step's tensors and the four feature maps used for camera 11 (after ten other cameras of the step) are bit-identical to those a fresh
  step plan produces for that camera alone; the bits do not depend on the call count or on the stream"""
  from dynibar_amd import nvidia_eval
  H, W, N, render_idx = 16, 20, 14, 5
  scene, model, args = ec.device_scene(DEV, H, W, N), _model(), ec.args_of(True)
  plan = scene.eval_step_plan(render_idx, args)
  step = scene.assemble_eval_step(plan)
  with torch.no_grad():
    coarse, fine = nvidia_eval.encode_step(model, step)
  last = None
  for cam in range(ec.NUM_CAMERAS):
    if cam != render_idx % ec.NUM_CAMERAS:
      last = scene.eval_sampler(step, scene.eval_view_plan(plan, cam)).get_all()
  shared = [(k, v) for k, v in sorted(last.items()) if isinstance(v, torch.Tensor)]
  shared += [('masked', step.static_src_rgbs_masked), ('ref_time', step.ref_time), ('coarse ref', coarse[0]), ('coarse static', coarse[2]),
             ('fine ref', fine[0]), ('fine static', fine[2])]
  fresh = _step_bits(scene, model, render_idx, args, 11)[2]
  torch.cuda.synchronize()
  _assert_same_bits(shared, fresh, 'camera 11 of a shared step against a fresh step')
  assert float(coarse[0].std()) > 0 and bool(torch.isfinite(fine[2]).all())
  side, busy = torch.cuda.Stream(), torch.cuda.Stream()
  with torch.cuda.stream(side):
    third = _step_bits(scene, model, render_idx, args, 11)[2]
  torch.cuda.synchronize()
  with torch.cuda.stream(busy):
    for _ in range(4):
      scene.assemble_eval_step(scene.eval_step_plan(N - 4, args))
  fourth = _step_bits(scene, model, render_idx, args, 11)[2]
  with torch.cuda.stream(busy):
    for _ in range(4):
      scene.assemble_eval_step(scene.eval_step_plan(N - 4, args))
  torch.cuda.synchronize()
  _assert_same_bits(third, fresh, 'a side stream')
  _assert_same_bits(fourth, fresh, 'while another step assembles on a second stream')


def _render_args(**more):
  return ec.args_of(True, anti_alias_pooling=0, mask_rgb=1, occ_weights_mode=0, chunk_size=128, N_samples=8, N_importance=8, inv_uniform=True,
                    white_bkgd=False, **more)


def test_copies_and_no_synchronisation():
  """test_one_copy_and_no_synchronisation of test_gpu_bullet.py for this path.  After a warm-up step: the assembly of a step and of its
  views raises nothing under sync debug mode 'error' and moves data once per step (16 V + 8 bytes from the pinned staging buffer) and once
  per view (136 bytes), nothing back.  A whole ``views`` step is then compared with the same eleven renders alone: it adds exactly one
  device-to-host copy (the table, into pinned memory), no host-to-device copy and no synchronising call that torch reports -- its one wait
  is the event's, before the first yield."""
  from dynibar_amd import nvidia_eval, projection, sample_ray
  H, W, N, render_idx = 16, 20, 14, 5
  a = ec.make_scene(H, W, N)
  scene, model, args = ec.device_scene(DEV, H, W, N), _model(), _render_args()
  projector = projection.Projector(DEV)
  warm = list(nvidia_eval.views(scene, model, projector, args, render_idx))
  assert len(warm) == 11
  torch.cuda.synchronize()
  torch.cuda.set_sync_debug_mode('error')
  try:
    for _ in range(3):  # (with the views more copies than staging slots: a slot is reused without a wait)
      plan = scene.eval_step_plan(render_idx, args)
      step = scene.assemble_eval_step(plan)
      for cam in (0, 11):
        got = scene.eval_sampler(step, scene.eval_view_plan(plan, cam)).get_all()
      pair = scene.eval_mask_pair(render_idx, 11)
  finally:
    torch.cuda.set_sync_debug_mode('default')
  data = ec.collated(ec.restate_item(a, render_idx, 11, True, ec.bounds_of(a, np.float32)))
  sc.assert_same_batch(got, sample_ray.RaySamplerSingleImage(data, DEV).get_all(), 'evaluation view under sync debug mode')
  assert bool(torch.isfinite(pair).all())
  with _Copies() as seen:
    plan = scene.eval_step_plan(render_idx, args)
    step = scene.assemble_eval_step(plan)
  V = sum(plan['counts'])
  print('  step assembly: host-to-device', seen.h2d, 'device-to-host', seen.d2h)
  assert len(seen.h2d) == 1 and seen.h2d[0][0].startswith('aten.copy_') and seen.h2d[0][1] == [4 * (4 * V + 2)], seen.h2d
  assert seen.d2h == [], seen.d2h
  with _Copies() as seen:
    scene.eval_sampler(step, scene.eval_view_plan(plan, 0)).get_all()
    scene.eval_mask_pair(render_idx, 0)
  print('  view: host-to-device', seen.h2d, 'device-to-host', seen.d2h)
  assert len(seen.h2d) == 1 and seen.h2d[0][1] == [4 * 34] and seen.d2h == [], (seen.h2d, seen.d2h)
  with _Copies() as host_seen:
    sample_ray.RaySamplerSingleImage(data, DEV).get_all()
  print(f'  host sampler: {len(host_seen.h2d)} host-to-device copies of {sum(sum(b) for _, b in host_seen.h2d)} bytes per view')
  assert len(host_seen.h2d) >= 6  # (the counter sees the copies of the path this one replaces)
  # a whole step of the loop, against the same renders alone: the renderer (unchanged here) reads the image size back once per projection
  # context (ops.py, ``self.cams[0, :2].tolist()``) and uploads a few constants, so its own traffic is counted first
  def watched(fn):
    torch.cuda.set_sync_debug_mode('warn')
    try:
      with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        with _Copies() as seen:
          out = fn()
    finally:
      torch.cuda.set_sync_debug_mode('default')
    return out, seen, [(str(w.message), w.filename, w.lineno) for w in caught if 'synchroniz' in str(w.message).lower()]

  def renders_alone():
    on_device = _render_args(frame_outputs='device')
    plan = scene.eval_step_plan(render_idx, args)
    with torch.no_grad():
      step = scene.assemble_eval_step(plan)
      featmaps = nvidia_eval.encode_step(model, step)
      for cam in range(ec.NUM_CAMERAS):
        if cam != render_idx % ec.NUM_CAMERAS:
          nvidia_eval.render_view(scene, step, scene.eval_view_plan(plan, cam), featmaps, model, projector, args, on_device)

  _, base, base_syncs = watched(renders_alone)
  rows, seen, syncs = watched(lambda: list(nvidia_eval.views(scene, model, projector, args, render_idx)))
  staged = lambda c: sorted(b for f, b in c.h2d if f.startswith('aten.copy_') and b in ([4 * (4 * V + 2)], [4 * 34]))
  print(f'  renders alone: {len(base_syncs)} synchronising calls, {len(base.h2d)} host-to-device, {len(base.d2h)} device-to-host {sorted(set(base.d2h))}')
  print(f'  views: {len(syncs)} synchronising calls, {len(seen.h2d)} host-to-device, {len(seen.d2h)} device-to-host')
  assert rows == warm, 'a second pass over the step gives the same numbers'
  assert staged(seen) == staged(base) == sorted([[4 * (4 * V + 2)]] + [[4 * 34]] * 11), (staged(seen), staged(base))
  assert len(seen.h2d) == len(base.h2d), 'the mask pairs, the metrics and the table add no host-to-device copy'
  assert len(seen.d2h) == len(base.d2h) + 1 and sorted(seen.d2h) == sorted(base.d2h + ['aten.copy_.default']), (seen.d2h, base.d2h)
  assert len(syncs) == len(base_syncs), f'views adds synchronising calls to the renders\' own: {syncs} against {base_syncs}'


@pytest.mark.parametrize('H,W', [(7, 7), (9, 13), (17, 19)])
@pytest.mark.parametrize('C', [1, 3])
def test_mask_pair_equals_numpy(H, W, C):
  """a random 0 / 1 mask, the all-zero and the all-one mask: (m, 1 - m) exactly, every element written"""
  ec.check_mask_pair(DEV, H, W, C)


def test_entry_points_refuse_untouched():
  """both new entry points refuse before a launch, set dyn_last_error and leave their outputs untouched; the evaluation scene refuses the
  training and the bullet-time calls; a valid call afterwards still gives the right bits"""
  ec.check_entry_refusals(DEV)
  ec.check_scene_refusals(ec.device_scene(DEV, 17, 19, 14))
  torch.cuda.synchronize()
  ec.check_get_all(DEV, 17, 19, 14, True)


def test_one_time_step_end_to_end():
  """16 x 20 (16 is the encoder's minimum, the metrics need 7), N = 14, synthetic weights, 8 + 8 samples, one time step.  For two cameras the
  frame rendered from the device sampler (kept on the device) equals the host sampler's on the restated item in rgb and depth of
  outputs_fine_ref, bit for bit.  The numbers ``views`` yields for every camera of the step equal ``nvidia_frame_metrics`` on the host path's
  frame exactly (the kernels are deterministic: no tolerance), and ``evaluate`` over that step returns their means."""
  from dynibar_amd import metrics, nvidia_eval, projection, render_image, sample_ray
  H, W, N, render_idx = 16, 20, 14, 5
  a = ec.make_scene(H, W, N)
  scene, model, args = ec.device_scene(DEV, H, W, N), _model(), _render_args()
  projector = projection.Projector(DEV)
  bounds = ec.bounds_of(a, np.float32)

  def host_frame(cam):
    """eval_nvidia.py:323-378 on the host sampler, then :380-457 through nvidia_frame_metrics"""
    data = ec.collated(ec.restate_item(a, render_idx, cam, True, bounds))
    with torch.no_grad():
      ray_sampler = sample_ray.RaySamplerSingleImage(data, device=DEV)
      ray_batch = ray_sampler.get_all()
      cb_featmaps_1, _ = model.feature_net(ray_batch['src_rgbs'].squeeze(0).permute(0, 3, 1, 2))
      static_src_rgbs = ray_batch['static_src_rgbs'].squeeze(0).permute(0, 3, 1, 2)
      _, static_featmaps = model.feature_net(static_src_rgbs)
      cb_featmaps_1_fine, _ = model.feature_net_fine(ray_batch['src_rgbs'].squeeze(0).permute(0, 3, 1, 2))
      static_src_rgbs_ = static_src_rgbs * ray_batch['static_src_masks'].squeeze(0)[:, None, ...]
      _, static_featmaps_fine = model.feature_net_fine(static_src_rgbs_)
      idx = int(data['id'].item())
      offsets = [int(i - idx) for i in data['nearest_pose_ids'].squeeze().tolist()]
      ret = render_image.render_single_image_nvi(
          frame_idx=(idx, None), time_embedding=(data['ref_time'].to(DEV), None), time_offset=(offsets, None), ray_sampler=ray_sampler,
          ray_batch=ray_batch, model=model, projector=projector, chunk_size=args.chunk_size, det=True, N_samples=args.N_samples, args=args,
          inv_uniform=args.inv_uniform, N_importance=args.N_importance, white_bkgd=args.white_bkgd,
          coarse_featmaps=(cb_featmaps_1, None, static_featmaps), fine_featmaps=(cb_featmaps_1_fine, None, static_featmaps_fine), is_train=False)
    rgb, depth = ret['outputs_fine_ref']['rgb'], ret['outputs_fine_ref']['depth']
    numbers = metrics.nvidia_frame_metrics(rgb, a['gt_views'][render_idx, cam], a['gt_masks'][render_idx, cam])
    return rgb, depth, numbers

  plan = scene.eval_step_plan(render_idx, args)
  step = scene.assemble_eval_step(plan)
  with torch.no_grad():
    featmaps = nvidia_eval.encode_step(model, step)
  on_device = _render_args(frame_outputs='device')
  want = {}
  for cam in range(ec.NUM_CAMERAS):
    if cam == render_idx % ec.NUM_CAMERAS:
      continue
    rgb, depth, want[cam] = host_frame(cam)
    if cam in (0, 11):
      with torch.no_grad():
        ret, _ = nvidia_eval.render_view(scene, step, scene.eval_view_plan(plan, cam), featmaps, model, projector, args, on_device)
      for k, h in (('rgb', rgb), ('depth', depth)):
        d = ret['outputs_fine_ref'][k]
        assert h.device.type == 'cpu' and d.is_cuda and tuple(h.shape) == tuple(d.shape) and d.dtype == torch.float32, k
        assert torch.equal(h.view(torch.int32), d.cpu().view(torch.int32)), f'camera {cam}: {k} differs between the device-fed and the host-fed frame'
      assert bool(torch.isfinite(rgb).all()) and float(rgb.std()) > 1e-3, 'the rendered frame must not be flat'
  keys = nvidia_eval.NUMBERS + ('valid_fraction',)
  got = list(nvidia_eval.views(scene, model, projector, args, render_idx))
  assert [v['cam'] for v in got] == sorted(want) and len(got) == 11
  for v in got:
    print('  camera', v['cam'], {k: v[k] for k in keys})
    assert v['render_idx'] == render_idx and v['rgb_path'] == 'mv_images/%05d/cam%02d.jpg' % (render_idx, v['cam'] + 1)
    assert {k: v[k] for k in keys} == want[v['cam']], f'camera {v["cam"]}: {v} != {want[v["cam"]]}'
  assert 0.0 < got[0]['valid_fraction'] <= 1.0 and got[0]['psnr'] != got[1]['psnr']
  seen = []
  result = nvidia_eval.evaluate(scene, model, projector, args, steps=[render_idx], on_step=lambda idx, moving: seen.append((idx, moving)))
  assert result['views'] == got
  for k in nvidia_eval.NUMBERS:
    assert result[k] == float(np.mean(np.array([want[c][k] for c in sorted(want)]))), k
  assert len(seen) == 1 and seen[0][0] == render_idx and seen[0][1] == {k: result[k] for k in nvidia_eval.NUMBERS}
