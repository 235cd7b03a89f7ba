"""Host-side checks of the frame metrics (dynibar_amd.metrics, csrc/dyn_metrics.h): the yardstick's own error (restatement (A) against the
exact form (E), with the float32 form (B) printed beside it), the restated PSNR against what the REAL reference's calculate_psnr returns
(tests/golden/eval_metrics.npz), the C-ABI entries without a device, and the refusal to run without one.

SSIM has no golden from the reference: its calculate_ssim calls skimage, which is not installed where the goldens are made.  The SSIM checks
rest on the restatement of skimage's published algorithm (tests/metrics_restatement.py), and the reference's implicit data_range is unverified."""
import ctypes
import os

import numpy as np
import pytest
import torch

import metrics_restatement as mr
import parity
from dynibar_amd import _lib

SHAPES = [(7, 7), (8, 300), (40, 56), (288, 512)]


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('name', mr.PREDICTIONS)
def test_float64_restatement_against_the_exact_form(H, W, name):
  """(A) stays within B(R) of (E) on every case and element (scipy's running sums: up to 8e-12 on `bright`); (B), the float32 form, is
  printed for the record: it is orders of magnitude above the limit, so float accumulation anywhere in the kernel fails the GPU check"""
  c = mr.make_case(H, W, name)
  a, b, _ = mr.prepare(c['pred'], c['target'] if c['target_u8'] is None else c['target_u8'])
  means = mr.exact_means(a, b)
  for R in (1.0, 2.0):
    E = mr.ssim_map_exact(a, b, R, means)
    err = np.abs(mr.ssim_map_uniform(a, b, R) - E).astype(np.float64)
    err32 = np.abs(mr.ssim_map_uniform(a, b, R, np.float32) - E).astype(np.float64)
    B = mr.map_limit(R)
    print(f'  [{H}x{W} {name} R={R:g}] float64 form: {err.max():.3e} of {B:.3e}; float32 form: {err32.max():.3e}')
    parity.record_margin(f'metrics restatement (A) vs exact [{H}x{W} {name} R={R:g}]', torch.from_numpy(err.reshape(-1)),
                         torch.full((1,), B, dtype=torch.float64).expand(err.size))
    assert (err <= B).all()
    if name == 'identical':
      assert (E == 1).all()


def test_map_limit_values():
  assert abs(mr.map_limit(1.0) - 1.8e-11) < 0.1e-11 and abs(mr.map_limit(2.0) - 4.4e-12) < 0.1e-12


def test_case_generator_covers_the_threshold():
  """the band holds sums exactly at float32(1e-3) (not valid), one ulp either side, and triples whose decision depends on the order"""
  c = mr.make_case(40, 56, 'noisy')
  band = c['pred'][20]
  t = np.float32(1e-3)
  s1, s2 = (band[:, 0] + band[:, 1]) + band[:, 2], band[:, 0] + (band[:, 1] + band[:, 2])
  assert (s1 == t).any() and (s1 == np.nextafter(t, np.float32(0))).any() and (s1 == np.nextafter(t, np.float32(1))).any()
  assert ((s1 > t) != (s2 > t)).sum() >= 8
  valid = mr.prepare(c['pred'], c['target'])[2]
  np.testing.assert_array_equal(valid[20, :, 0], (s1 > t).astype(np.float32))  # numpy's sum over the last axis is (r + g) + b
  assert (valid[20, s1 == t] == 0).all()
  assert (c['pred'][:5, :7] == 0).all() and (valid[:5, :7] == 0).all()


def test_restated_psnr_against_the_reference_golden(golden_dir):
  """calculate_psnr of the real reference on the recorded inputs: the restatement (and the expressions dynibar_amd.metrics applies to the
  device's sums) within 4.35 * (N + 4) * 2^-53 dB (a reordered double sum of N non-negative terms, through 10 log10); 0 where mse == 0"""
  from dynibar_amd import metrics
  g = np.load(os.path.join(golden_dir, 'eval_metrics.npz'))
  assert tuple(g['predictions']) == mr.PREDICTIONS and tuple(g['masks']) == mr.MASKS
  for name in mr.PREDICTIONS:
    gt, pred = g[f'{name}/gt'], g[f'{name}/pred']
    N = gt.size
    lim = 4.35 * (N + 4) * 2.0 ** -53
    for k in mr.MASKS:
      m, want = g[f'{name}/mask/{k}'], float(g[f'{name}/psnr/{k}'])
      got = mr.calculate_psnr_restated(gt, pred, m)
      sse, _, msum = mr.masked_sums_exact(gt, pred, np.zeros(gt.shape), m)
      got2 = metrics._psnr_of(float(sse), float(msum))
      parity.record_margin(f'restated psnr vs reference golden [{name} {k}]', max(abs(got - want), abs(got2 - want)), lim)
      assert abs(got - want) <= lim and abs(got2 - want) <= lim, f'{name} {k}: {got!r} / {got2!r} against the reference\'s {want!r}'
      if name == 'identical' or k == 'zero':
        assert want == 0 and got == 0 and got2 == 0
  assert float(g['noisy/psnr/ones']) > 10


def test_new_symbols_are_exported_and_declared():
  lib = _lib.lib()
  for name in ('dyn_frame_metrics_workspace_bytes', 'dyn_frame_metrics'):
    assert hasattr(lib, name) and name in _lib._FUNC_SPECS
  assert 'DynFrameMetricsParams' in _lib.STRUCTS
  fields = dict(_lib._STRUCT_SPECS['DynFrameMetricsParams'])
  assert fields['data_range'] is ctypes.c_double and fields['valid'] is ctypes.c_void_p and fields['workspace_bytes'] is ctypes.c_size_t
  names = [lib.dyn_profile_name(i).decode() for i in range(lib.dyn_profile_count())]
  assert 'k_metrics_tile' in names and 'k_metrics_finish' in names


def _params(**kw):
  base = dict(H=9, W=13, M=1, pred=8, target=8, masks=8, mask_stride=9 * 13 * 3, mask_channels=3, data_range=1.0, workspace=8, workspace_bytes=1 << 20)
  base.update(kw)
  return _lib.params('DynFrameMetricsParams', **base)


def test_argument_errors_without_a_device():
  lib = _lib.lib()
  err = lambda: lib.dyn_last_error().decode()
  assert lib.dyn_frame_metrics(None, 8, None) == -1 and 'dyn_frame_metrics: null params' in err()
  with pytest.raises(RuntimeError, match='dyn_frame_metrics failed'):
    _lib.call('dyn_frame_metrics', None, None, None)
  for kw, msg in ((dict(H=6), '7 x 7 window'), (dict(W=6), '7 x 7 window'), (dict(H=1 << 15, W=1 << 15), 'too large'), (dict(M=0), 'M=0 masks'),
                  (dict(M=9), 'M=9 masks'), (dict(data_range=0.0), 'data_range'), (dict(data_range=-1.0), 'data_range'),
                  (dict(data_range=float('nan')), 'data_range'), (dict(data_range=float('inf')), 'data_range'), (dict(pred=None), 'are required'),
                  (dict(target=None), 'are required'), (dict(masks=None), 'masks is required'), (dict(mask_channels=2), 'mask_channels=2'),
                  (dict(M=2, mask_stride=10), 'mask_stride'), (dict(workspace=None), 'workspace'), (dict(workspace_bytes=16), 'workspace of 16 bytes'),
                  (dict(workspace=12), '8-byte aligned')):
    assert lib.dyn_frame_metrics(_params(**kw), 8, None) == -1, kw
    assert msg in err(), (kw, err())
  assert lib.dyn_frame_metrics(_params(), None, None) == -1 and 'are required' in err()
  assert lib.dyn_frame_metrics(_params(), 12, None) == -1 and '8-byte aligned' in err()
  # the valid mask alone needs no masks pointer: the call gets past the argument checks only with one
  assert lib.dyn_frame_metrics(_params(masks=None, valid_as_mask0=1, workspace_bytes=0), 8, None) == -1 and 'workspace of 0 bytes' in err()


def test_workspace_size():
  lib = _lib.lib()
  f = lib.dyn_frame_metrics_workspace_bytes
  assert f(6, 13, 1) == 0 and f(13, 6, 1) == 0 and f(9, 13, 0) == 0 and f(9, 13, 9) == 0 and f(1 << 15, 1 << 15, 1) == 0 and f(-1, 9, 1) == 0
  assert f(7, 7, 1) > 0 and f(7, 7, 1) % 8 == 0
  sizes = [f(h, w, m) for h, w, m in ((7, 7, 1), (7, 7, 2), (40, 56, 2), (288, 512, 2), (288, 512, 3), (1080, 1920, 3), (1080, 1920, 8))]
  assert all(a < b for a, b in zip(sizes, sizes[1:]))
  for h, w, m in ((7, 7, 1), (40, 56, 3), (288, 512, 8)):  # monotone in each argument
    assert f(h + 64, w, m) >= f(h, w, m) and f(h, w + 64, m) >= f(h, w, m) and (m == 8 or f(h, w, m + 1) > f(h, w, m))


def test_no_cpu_fallback():
  """host inputs are uploaded, never computed on the host: without a device the entry points raise"""
  from dynibar_amd import metrics
  a = np.zeros((9, 13, 3), np.float32)
  if torch.cuda.is_available():  # (the suite also runs where a device is present: there the same call is uploaded and answered)
    assert metrics.calculate_psnr(a, a, a) == 0
    return
  for call in (lambda: metrics.calculate_psnr(a, a, a), lambda: metrics.calculate_ssim(a, a, a),
               lambda: metrics.structural_similarity(a, a, data_range=1.0), lambda: metrics.nvidia_frame_metrics(a, a, a)):
    with pytest.raises(RuntimeError, match='HIP device'):
      call()
  with pytest.raises(ValueError, match='same dimensions'):  # the reference's check comes first
    metrics.calculate_ssim(a, a[:8], a)
