"""The LPIPS kernels (dynibar_amd/csrc/dyn_lpips.h, dynibar_amd/lpips.py) on the MI355X against tests/lpips_restatement.py through
tests/lpips_cases.py (which states every limit): the preparation bit for bit, the five maps and the number against float64 within twice
the float32 restatement's own pooled distance, six masks against longdouble sums of the device's own maps, identical images exactly 0,
independence of a mask from its neighbours, bitwise determinism across calls and streams with a poisoned workspace, the three kinds of
input and the one synchronisation of ``nvidia_frame_metrics(..., lpips=net)``, one time step of ``nvidia_eval`` with a network, and the
ValueErrors.  Shapes: 31 x 31 (every map at its minimum, every window touches padding), 32 x 45 (stride-4 and pool remainders), 67 x 95
(nothing divides a 32-lane tile), 288 x 512 (the evaluation's shape) once per check that needs it."""
import warnings

import numpy as np
import pytest
import torch

import lpips_cases as lc
import lpips_restatement as lr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL = lr.SHAPES[:3]


@pytest.mark.parametrize('H,W', SMALL)
@pytest.mark.parametrize('kind', lr.PAIRS)
def test_preparation_bit_exact(H, W, kind):
  lc.check_preparation(DEV, H, W, kind)


def test_preparation_bit_exact_at_the_evaluation_shape():
  lc.check_preparation(DEV, 288, 512, 'border')


@pytest.mark.parametrize('H,W', lr.SHAPES)
@pytest.mark.parametrize('kind', lr.PAIRS)
@pytest.mark.parametrize('seed', lc.SEEDS)
def test_accuracy_against_float64(H, W, kind, seed):
  """check 2: every tap's map and the number, within twice the float32 restatement's pooled distance from float64 (lpips_cases)"""
  lc.check_accuracy(DEV, H, W, kind, seed, lr.SHAPES)


@pytest.mark.parametrize('H,W', SMALL)
@pytest.mark.parametrize('kind', lr.PAIRS)
def test_masks(H, W, kind):
  lc.check_masks(DEV, H, W, kind)


def test_masks_at_the_evaluation_shape():
  lc.check_masks(DEV, 288, 512, 'border')


@pytest.mark.parametrize('H,W', lr.SHAPES)
def test_identical_images_give_exactly_zero(H, W):
  lc.check_identical(DEV, H, W)


@pytest.mark.parametrize('H,W', [(67, 95), (288, 512)])
def test_a_masks_sums_do_not_depend_on_its_neighbours(H, W):
  lc.check_independence(DEV, H, W)


def _frame(H, W, kind):
  r = lc.reference(H, W, kind, 0)
  ms = lr.make_masks(H, W)
  pred, tgt = lc.dev_t(r['pred'], DEV), lc.dev_t(r['target'], DEV)
  masks = torch.stack([lc.dev_t(ms[k], DEV) for k in ('dynamic', 'static', 'fractional')]).contiguous()
  return lambda: lc.net_of(0).frame_sums(pred, tgt, masks, apply_valid=True, valid_as_mask0=True, want_maps=True)


@pytest.mark.parametrize('H,W', [(67, 95), (288, 512)])
def test_bitwise_determinism_across_calls_and_streams(H, W):
  """check 6: two calls, a call on a side stream, and a call issued while the same kernels run on a second stream for another frame; the
  workspace starts as NaN under the suite (DYNIBAR_TRAIN_POISON, tests/conftest.py): every value read was written by this call"""
  from dynibar_amd.train_static import POISON_SCRATCH
  assert POISON_SCRATCH
  run, other = _frame(H, W, 'noisy'), _frame(H, W, 'close')
  first = run()
  second = run()
  torch.cuda.synchronize()
  side, busy = torch.cuda.Stream(), torch.cuda.Stream()
  with torch.cuda.stream(side):
    third = run()
  torch.cuda.synchronize()
  with torch.cuda.stream(busy):
    for _ in range(4):
      other()
  fourth = run()
  with torch.cuda.stream(busy):
    for _ in range(4):
      other()
  torch.cuda.synchronize()
  for tag, o in (('second call', second), ('side stream', third), ('beside another frame', fourth)):
    lc.assert_bits(o['sums'].cpu().numpy(), first['sums'].cpu().numpy(), f'sums, {tag}')
    for l in range(5):
      lc.assert_bits(o['maps'][l].cpu().numpy(), first['maps'][l].cpu().numpy(), f'map {l + 1}, {tag}')
  s = first['sums'].cpu().numpy()
  assert np.isfinite(s).all() and (s[0, :, 0] > 0).all()


@pytest.mark.parametrize('H,W', [(32, 45), (288, 512)])
def test_entry_points_numpy_and_tensors(H, W):
  """check 7, first part"""
  lc.check_inputs(DEV, H, W)


def test_no_synchronisation_but_the_final_copy():
  """check 7, second part: with device inputs the kernel path raises nothing under torch's sync debug mode 'error'; the whole of
  nvidia_frame_metrics with a network synchronises exactly once, for its one copy of both tables"""
  from dynibar_amd import lpips, metrics
  H, W = 288, 512
  r = lc.reference(H, W, 'noisy', 0)
  net = lc.net_of(0)
  pred, tgt, dyn = lc.dev_t(r['pred'], DEV), lc.dev_t(r['target'], DEV), lc.dev_t(lr.make_masks(H, W)['dynamic'], DEV)
  plain = metrics.nvidia_frame_metrics(pred, tgt, dyn)
  want = metrics.nvidia_frame_metrics(pred, tgt, dyn, lpips=net)  # (first call: the packed weights go to the device)
  torch.cuda.synchronize()
  torch.cuda.set_sync_debug_mode('error')
  try:
    masks = torch.stack([dyn, 1 - dyn]).contiguous()
    out = net.frame_sums(pred, tgt, masks, apply_valid=True, valid_as_mask0=True, want_maps=True)
  finally:
    torch.cuda.set_sync_debug_mode('default')
  rows = out['sums'].cpu().tolist()
  assert [lpips.lpips_of(t) for t in rows] == [want['lpips'], want['dynamic_lpips'], want['static_lpips']]
  torch.cuda.set_sync_debug_mode('warn')
  try:
    with warnings.catch_warnings(record=True) as seen:
      warnings.simplefilter('always')
      got = metrics.nvidia_frame_metrics(pred, tgt, dyn, lpips=net)
  finally:
    torch.cuda.set_sync_debug_mode('default')
  syncs = [w for w in seen if 'synchroniz' in str(w.message).lower()]
  print('  synchronising calls of nvidia_frame_metrics with a network:', [(w.filename, w.lineno) for w in syncs])
  assert len(syncs) == 1, [(str(w.message), w.filename, w.lineno) for w in seen]
  assert got == want and {k: got[k] for k in plain} == plain and 0 < got['dynamic_lpips'] and 0 < got['static_lpips']


def test_one_time_step_of_nvidia_eval_with_a_network():
  """check 8: the synthetic evaluation scene of tests/eval_scene_cases.py at 32 x 36 (LPIPS needs 31), one time step: ``views(..., lpips=net)``
  yields the three new keys, equal to ``net.frame_sums`` on the same frames; the six old keys equal the run without ``lpips=``; the step makes
  the same single device-to-host copy; ``evaluate`` adds the three means"""
  import eval_scene_cases as ec
  from test_gpu_bullet import _Copies
  from test_gpu_eval_scene import _model, _render_args
  from dynibar_amd import lpips, metrics, nvidia_eval, projection
  H, W, N, render_idx = 32, 36, 14, 5
  scene, model, args = ec.device_scene(DEV, H, W, N), _model(), _render_args()
  projector = projection.Projector(DEV)
  net = lc.net_of(0)
  old = list(nvidia_eval.views(scene, model, projector, args, render_idx))
  warm = list(nvidia_eval.views(scene, model, projector, args, render_idx, lpips=net))
  with _Copies() as base:
    old2 = list(nvidia_eval.views(scene, model, projector, args, render_idx))
  with _Copies() as seen:
    new = list(nvidia_eval.views(scene, model, projector, args, render_idx, lpips=net))
  assert old2 == old and new == warm and len(new) == 11
  # the step's one device-to-host copy is the table's, into pinned memory (aten.copy_); every other transfer is the renderer's own (it reads the
  # image size back per projection context, a count that varies by one from pass to pass with and without a network): the metrics add none
  print('  plain step:', len(base.h2d), 'host-to-device,', sorted(set(base.d2h)), len(base.d2h), '| with a network:', len(seen.h2d), sorted(set(seen.d2h)), len(seen.d2h))
  assert seen.d2h.count('aten.copy_.default') == 1 == base.d2h.count('aten.copy_.default') and set(seen.d2h) == set(base.d2h)
  assert len(seen.h2d) == len(base.h2d)
  cam = new[0]['cam']
  frame = torch.rand(H, W, 3, device=DEV)
  with _Copies() as own:
    pair = scene.eval_mask_pair(render_idx, cam)
    table = metrics.frame_sums(frame, scene.gt_view(render_idx, cam), pair, data_range=2.0, apply_valid=True, valid_as_mask0=True)['sums']
    taps = net.frame_sums(frame, scene.gt_view(render_idx, cam), pair, apply_valid=True, valid_as_mask0=True)['sums']
  assert own.h2d == [] and own.d2h == [], (own.h2d, own.d2h)
  assert bool(torch.isfinite(table).all()) and bool(torch.isfinite(taps).all())
  for o, v in zip(old, new):
    assert set(v) == set(o) | set(nvidia_eval.LPIPS_NUMBERS) and {k: v[k] for k in o} == o
  plan = scene.eval_step_plan(render_idx, args)
  on_device = _render_args(frame_outputs='device')
  with torch.no_grad():
    step = scene.assemble_eval_step(plan)
    featmaps = nvidia_eval.encode_step(model, step)
    for v in new[:3]:
      ret, _ = nvidia_eval.render_view(scene, step, scene.eval_view_plan(plan, v['cam']), featmaps, model, projector, args, on_device)
      rows = net.frame_sums(ret['outputs_fine_ref']['rgb'].contiguous(), scene.gt_view(render_idx, v['cam']), scene.eval_mask_pair(render_idx, v['cam']),
                            apply_valid=True, valid_as_mask0=True)['sums'].cpu().tolist()
      print('  camera', v['cam'], {k: v[k] for k in nvidia_eval.LPIPS_NUMBERS})
      assert [v[k] for k in nvidia_eval.LPIPS_NUMBERS] == [lpips.lpips_of(t) for t in rows]
      assert all(isinstance(v[k], float) for k in nvidia_eval.LPIPS_NUMBERS) and v['lpips'] > 0
  seen_steps = []
  result = nvidia_eval.evaluate(scene, model, projector, args, steps=[render_idx], on_step=lambda i, moving: seen_steps.append((i, moving)), lpips=net)
  assert result['views'] == new
  for k in nvidia_eval.NUMBERS + nvidia_eval.LPIPS_NUMBERS:
    assert result[k] == float(np.mean(np.array([v[k] for v in new]))), k
  assert set(seen_steps[0][1]) == set(nvidia_eval.NUMBERS + nvidia_eval.LPIPS_NUMBERS)
  plain = nvidia_eval.evaluate(scene, model, projector, args, steps=[render_idx])
  assert set(plain) == set(nvidia_eval.NUMBERS) | {'views'} and plain['views'] == old


def test_value_errors():
  lc.check_value_errors(DEV)
