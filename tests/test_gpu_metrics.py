"""The frame metrics on the MI355X (dynibar_amd/metrics.py, csrc/dyn_metrics.h) against tests/metrics_restatement.py: the preparation bit for
bit against numpy, every element of the SSIM map against the exact (longdouble) form within B(R) = 144 * 2^-53 / C2(R), the masked sums and
the six numbers of a frame with the reference's expressions, the entry points with numpy / host / device inputs, bitwise determinism across
calls, streams and mask counts, no synchronisation but the final copy, and the ValueErrors.  (metrics_cases.py states every limit.)

SSIM has no golden from the reference (its calculate_ssim needs skimage, which is not installed where the goldens are made); PSNR has
(tests/test_metrics_cpu.py)."""
import warnings

import numpy as np
import pytest
import torch

import metrics_cases as mc
import metrics_restatement as mr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# the evaluation's shape; every window mostly reflection; one side barely above the window (twice); tile counts that do not divide, many partials
SHAPES = [(288, 512), (7, 7), (8, 300), (301, 9), (270, 480), (1080, 1920)]


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('name', mr.PREDICTIONS)
@pytest.mark.parametrize('R', mc.RANGES)
def test_frame_metrics(H, W, name, R):
  """checks 1-3: preparation bit-exact, the S map against the exact form, the sums of six masks and the six numbers of the frame"""
  mc.check_case(DEV, H, W, name, R)


@pytest.mark.parametrize('H,W', [(288, 512), (7, 7), (301, 9)])
def test_float_target_plain_masks_and_valid_as_mask0(H, W):
  mc.check_float_target_and_plain_masks(DEV, H, W)


@pytest.mark.parametrize('H,W', [(288, 512), (7, 7), (8, 300)])
@pytest.mark.parametrize('R', mc.RANGES)
def test_entry_points_numpy_and_tensors(H, W, R):
  """check 4: numpy inputs, host tensors and device tensors give the same bits"""
  mc.check_entry_points(DEV, H, W, R)


@pytest.mark.parametrize('H,W', [(288, 512), (270, 480)])
def test_a_masks_sums_do_not_depend_on_its_neighbours(H, W):
  mc.check_mask_independence(DEV, H, W)


def _frame(H, W, name):
  from dynibar_amd import metrics
  c = mr.make_case(H, W, name)
  pred, tgt = mc.dev_t(c['pred'], DEV), mc.dev_t(c['target'], DEV)
  masks = torch.stack([mc.dev_t(c['masks'][k], DEV) for k in ('dynamic', 'static', 'fractional')]).contiguous()
  run = lambda: metrics.frame_sums(pred, tgt, masks, data_range=2.0, apply_valid=True, valid_as_mask0=True, want_map=True)
  return run


@pytest.mark.parametrize('H,W', [(288, 512), (1080, 1920)])
def test_bitwise_determinism_across_calls_and_streams(H, W):
  """check 5: two calls, a call on a side stream, and a call issued while the same kernels run on a second stream for another frame"""
  run, other = _frame(H, W, 'noisy'), _frame(H, W, 'close')
  first = run()
  second = run()
  torch.cuda.synchronize()
  side, busy = torch.cuda.Stream(), torch.cuda.Stream()
  with torch.cuda.stream(side):
    third = run()
  torch.cuda.synchronize()
  with torch.cuda.stream(busy):
    for _ in range(8):
      other()
  fourth = run()
  with torch.cuda.stream(busy):
    for _ in range(8):
      other()
  torch.cuda.synchronize()
  for tag, o in (('second call', second), ('side stream', third), ('beside another frame', fourth)):
    for k in ('sums', 'ssim_map'):
      mc.assert_bits(o[k].cpu().numpy(), first[k].cpu().numpy(), f'{k}, {tag}')
  assert np.isfinite(first['sums'].cpu().numpy()).all()


def test_no_synchronisation_but_the_final_copy():
  """check 6: with device inputs the kernel path (mask preparation included) raises nothing under torch's sync debug mode 'error'; the
  whole of nvidia_frame_metrics synchronises exactly once, for its copy of the sums.  The workspace starts as NaN under the suite
  (DYNIBAR_TRAIN_POISON, tests/conftest.py): every partial is written before it is read."""
  from dynibar_amd import metrics
  from dynibar_amd.train_static import POISON_SCRATCH
  assert POISON_SCRATCH
  c = mr.make_case(288, 512, 'noisy')
  pred, tgt, dyn = mc.dev_t(c['pred'], DEV), mc.dev_t(c['target_u8'], DEV), mc.dev_t(c['masks']['dynamic'], DEV)
  want = metrics.nvidia_frame_metrics(pred, tgt, dyn)  # (first call: library load, allocator growth)
  torch.cuda.synchronize()
  torch.cuda.set_sync_debug_mode('error')
  try:
    masks = torch.stack([dyn, 1 - dyn]).contiguous()
    out = metrics.frame_sums(pred, tgt, masks, data_range=metrics.REFERENCE_DATA_RANGE, apply_valid=True, valid_as_mask0=True)
  finally:
    torch.cuda.set_sync_debug_mode('default')
  rows = out['sums'].cpu().tolist()
  assert metrics._psnr_of(rows[0][0], rows[0][2]) == want['psnr'] and metrics._ssim_of(rows[2][1], rows[2][2]) == want['static_ssim']
  torch.cuda.set_sync_debug_mode('warn')
  try:
    with warnings.catch_warnings(record=True) as seen:
      warnings.simplefilter('always')
      got = metrics.nvidia_frame_metrics(pred, tgt, dyn)
  finally:
    torch.cuda.set_sync_debug_mode('default')
  syncs = [w for w in seen if 'synchroniz' in str(w.message).lower()]
  print('  synchronising calls of nvidia_frame_metrics:', [(w.filename, w.lineno) for w in syncs])
  assert len(syncs) == 1, [(str(w.message), w.filename, w.lineno) for w in seen]
  assert got == want


def test_value_errors():
  mc.check_value_errors(DEV)
