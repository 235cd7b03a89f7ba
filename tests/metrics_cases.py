"""Checks of dynibar_amd.metrics shared by tests/emu/test_emu_metrics.py (the wave-level emulator) and tests/test_gpu_metrics.py (the
MI355X).  The yardstick is tests/metrics_restatement.py; every limit is derived there or below, none is taken from the code under test.

Limits, with N = H * W * 3 the element count:
* valid, the prepared images, uint8 -> float: bit-exact against numpy, no element left out.
* the S map, every element, against the exact form (E): B(R) = 144 * 2^-53 / C2(R) (metrics_restatement.map_limit).
* sum(m): a reordered double sum of N non-negative terms: N * 2^-53 relative.  sum((a - b)^2 m): its terms carry three more roundings:
  (N + 3) * 2^-53 relative.  sum(S m): B(R) per element plus the summation: (B(R) + (N + 1) * 2^-53) * sum(m) (|S| <= 1).
* SSIM numbers within B(R) + N * 2^-53 (+ 2^-50 for the divisions done in double on both sides); PSNR within 4.35 * (N + 4) * 2^-53 dB
  (the relative error of the squared-error sum and of sum(m), through 10 log10).
"""
import functools
import math

import numpy as np
import torch

import metrics_restatement as mr
import parity

EPS53 = mr.EPS53
RANGES = (1.0, 2.0)


def bits(x):
  """float32 / uint8 array -> integers to compare bit for bit (-0.0 != +0.0, NaN == the same NaN)"""
  x = np.ascontiguousarray(x)
  return x.view(np.int32) if x.dtype == np.float32 else (x.view(np.int64) if x.dtype == np.float64 else x)


def assert_bits(got, want, what):
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, f'{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}'
  bad = bits(got) != bits(want)
  assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} elements differ in their bits, first at {tuple(np.argwhere(bad)[0])}'


@functools.lru_cache(maxsize=2)
def exact(H, W, name):
  """the case, its numpy preparation (from the uint8 target where the case has one) and the R-independent part of (E)"""
  c = mr.make_case(H, W, name)
  tgt = c['target'] if c['target_u8'] is None else c['target_u8']
  a, b, valid = mr.prepare(c['pred'], tgt)
  return c, tgt, a, b, valid, mr.exact_means(a, b)


def dev_t(x, device):
  return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def check_case(device, H, W, name, R):
  """checks 1-3 and 8 of one case: preparation bit-exact, the map against (E), the sums of six masks and the numbers of nvidia_frame_metrics"""
  from dynibar_amd import metrics
  c, tgt, a, b, valid, means = exact(H, W, name)
  tag = f'metrics [{H}x{W} {name} R={R:g}]'
  N = H * W * 3
  masks = [c['masks'][k] for k in mr.MASKS]
  out = metrics.frame_sums(dev_t(c['pred'], device), dev_t(tgt, device), [dev_t(m, device) for m in masks], data_range=R, apply_valid=True,
                           want_map=True, want_valid=True, want_prepared=True)
  out = {k: v.cpu().numpy() for k, v in out.items()}
  # 1. the preparation, bit for bit
  assert_bits(out['valid'], valid[..., 0].astype(np.uint8), f'{tag} valid')
  assert_bits(out['pred'], a, f'{tag} prepared pred')
  assert_bits(out['target'], b, f'{tag} prepared target')
  # 2. the map, every element
  E = mr.ssim_map_exact(a, b, R, means)
  err = np.abs(out['ssim_map'].astype(np.longdouble) - E).astype(np.float64)
  B = mr.map_limit(R)
  print(f'  {tag}: map max err {err.max():.3e} of B(R) {B:.3e} ({err.max() / B:.3f})')
  parity.record_margin(f'{tag} ssim map vs exact', torch.from_numpy(err.reshape(-1)), torch.full((1,), B, dtype=torch.float64).expand(err.size))
  assert np.isfinite(out['ssim_map']).all() and (err <= B).all(), f'{tag}: S map off by {err.max():.3e} (limit {B:.3e}) at {np.unravel_index(err.argmax(), err.shape)}'
  if name == 'identical':
    assert (out['ssim_map'] == 1.0).all(), f'{tag}: the map of identical images is not exactly 1'
  # 3. the three sums of every mask
  for i, k in enumerate(mr.MASKS):
    sse, ssum, msum = (float(v) for v in mr.masked_sums_exact(a, b, E, masks[i]))
    g_sse, g_ssum, g_msum = (float(v) for v in out['sums'][i])
    tiny = 1e-300
    for what, got, want, lim in ((f'sum m', g_msum, msum, N * EPS53 * msum), (f'sum d2 m', g_sse, sse, (N + 3) * EPS53 * sse),
                                 (f'sum S m', g_ssum, ssum, (B + (N + 1) * EPS53) * msum)):
      print(f'  {tag} {k}: {what} {got!r} exact {want!r} err {abs(got - want):.3e} limit {lim:.3e}')
      parity.record_margin(f'{tag} {k} {what}', abs(got - want), max(lim, tiny))
      assert abs(got - want) <= lim, f'{tag} mask {k}: {what} = {got!r}, exact {want!r}, limit {lim:.3e}'
    if k == 'zero':
      assert (g_sse, g_ssum, g_msum) == (0.0, 0.0, 0.0)
      assert metrics._psnr_of(g_sse, g_msum) == 0 and metrics._ssim_of(g_ssum, g_msum) == 0
    if name == 'identical':
      assert g_sse == 0.0 and g_ssum == g_msum, f'{tag} mask {k}: identical images give sse {g_sse!r}, sum S m {g_ssum!r} against sum m {g_msum!r}'
      if k != 'fractional':
        assert g_msum == float(masks[i].astype(np.float64).sum())  # sums of 0 / 1 weights are exact in any order
  # ... and the six numbers of the frame, masks valid / dynamic / 1 - dynamic, with the reference's expressions on the exact sums
  dyn = c['masks']['dynamic']
  got = metrics.nvidia_frame_metrics(dev_t(c['pred'], device), dev_t(tgt, device), dev_t(dyn, device), data_range=R)
  lim_ssim, lim_psnr = B + N * EPS53 + 2.0 ** -50, 4.35 * (N + 4) * EPS53
  for prefix, m in (('', valid), ('dynamic_', dyn), ('static_', 1 - dyn)):
    sse, ssum, msum = mr.masked_sums_exact(a, b, E, m)
    want_p, want_s = mr.psnr_reference(sse, msum), mr.ssim_reference(ssum, msum)
    gp, gs = got[prefix + 'psnr'], got[prefix + 'ssim']
    print(f'  {tag} {prefix}psnr {gp!r} exact {want_p!r}; {prefix}ssim {gs!r} exact {want_s!r}')
    parity.record_margin(f'{tag} {prefix}psnr', abs(gp - want_p), lim_psnr)
    parity.record_margin(f'{tag} {prefix}ssim', abs(gs - want_s), lim_ssim)
    assert abs(gp - want_p) <= lim_psnr, f'{tag}: {prefix}psnr {gp!r} against {want_p!r} (limit {lim_psnr:.2e} dB)'
    assert abs(gs - want_s) <= lim_ssim, f'{tag}: {prefix}ssim {gs!r} against {want_s!r} (limit {lim_ssim:.2e})'
    if name == 'identical':
      ms = float(msum)
      assert gp == 0 and gs == ms / (ms + 1e-8), f'{tag}: identical images give {prefix}psnr {gp!r}, {prefix}ssim {gs!r}'
  assert got['valid_fraction'] == float(valid.mean(dtype=np.float64))
  assert set(got) == {'psnr', 'ssim', 'dynamic_psnr', 'dynamic_ssim', 'static_psnr', 'static_ssim', 'valid_fraction'}
  assert all(isinstance(v, (int, float)) for v in got.values())


def check_float_target_and_plain_masks(device, H, W, R=2.0):
  """a float32 target, a [H, W] mask next to [H, W, 3] ones, and valid_as_mask0: the same bits as the uint8 / explicit-mask form"""
  from dynibar_amd import metrics
  c, tgt, a, b, valid, _ = exact(H, W, 'noisy')
  pred, masks = dev_t(c['pred'], device), c['masks']
  ref = metrics.frame_sums(pred, dev_t(tgt, device), [dev_t(masks[k], device) for k in ('valid', 'dynamic', 'ones')], data_range=R, apply_valid=True)
  alt = metrics.frame_sums(pred, dev_t(c['target'], device), [dev_t(masks['dynamic'][..., 0], device), dev_t(masks['ones'], device)], data_range=R,
                           apply_valid=True, valid_as_mask0=True, want_prepared=True)
  assert_bits(alt['sums'].cpu().numpy(), ref['sums'].cpu().numpy(), 'float target / [H, W] mask / valid_as_mask0 against the explicit form')
  assert_bits(alt['target'].cpu().numpy(), b, 'prepared float target')
  raw = metrics.frame_sums(pred, dev_t(c['target'], device), [dev_t(masks['ones'], device)], data_range=R, want_prepared=True)
  assert_bits(raw['pred'].cpu().numpy(), c['pred'], 'apply_valid off leaves pred as it is')


def check_entry_points(device, H, W, R=2.0):
  """check 4: calculate_psnr / calculate_ssim / structural_similarity with numpy inputs, host tensors and device tensors: the same bits,
  and the reference's values"""
  from dynibar_amd import metrics
  c, tgt, a, b, valid, means = exact(H, W, 'close')
  m = c['masks']['fractional']
  N = H * W * 3
  forms = dict(numpy=lambda x: x, host=lambda x: torch.from_numpy(x), device=lambda x: dev_t(x, device))
  res = {}
  for k, f in forms.items():
    mean, smap = metrics.structural_similarity(f(b), f(a), data_range=R, full=True)
    res[k] = (metrics.calculate_psnr(f(b), f(a), f(m)), metrics.calculate_ssim(f(b), f(a), f(m), data_range=R),
              metrics.calculate_ssim(f(b), f(a), f(m)), mean, metrics.structural_similarity(f(b), f(a), data_range=R), smap)
    assert all(isinstance(v, float) for v in res[k][:5]) and isinstance(smap, np.ndarray) and smap.dtype == np.float64
  for k in ('host', 'device'):
    assert res[k][:5] == res['numpy'][:5], f'{k} inputs give {res[k][:5]}, numpy inputs {res["numpy"][:5]}'
    assert_bits(res[k][5], res['numpy'][5], f'structural_similarity map, {k} inputs')
  psnr, ssim, ssim_default, mean, mean2, smap = res['numpy']
  assert mean == mean2
  E = mr.ssim_map_exact(b, a, R, None)
  B = mr.map_limit(R)
  sse, ssum, msum = mr.masked_sums_exact(b, a, E, m)
  for what, got, want, lim in (('calculate_psnr', psnr, mr.psnr_reference(sse, msum), 4.35 * (N + 4) * EPS53),
                               ('calculate_ssim', ssim, mr.ssim_reference(ssum, msum), B + N * EPS53 + 2.0 ** -50),
                               ('structural_similarity mean', mean, float(E[3:-3, 3:-3].mean()), B + N * EPS53 + 2.0 ** -50)):
    print(f'  {what} [{H}x{W}]: {got!r} exact {want!r}')
    parity.record_margin(f'metrics {what} [{H}x{W}]', abs(got - want), lim)
    assert abs(got - want) <= lim, f'{what}: {got!r} against {want!r} (limit {lim:.2e})'
  err = np.abs(smap.astype(np.longdouble) - E).astype(np.float64)
  assert (err <= B).all()
  assert metrics.REFERENCE_DATA_RANGE == 2.0
  if R == metrics.REFERENCE_DATA_RANGE:
    assert ssim_default == ssim
  # the golden-free statement of calculate_psnr: against its line-by-line restatement
  want = mr.calculate_psnr_restated(b, a, m)
  assert abs(psnr - want) <= 4.35 * (N + 4) * EPS53


def check_mask_independence(device, H, W, R=1.0):
  """check 5, second half: M = 1 three times equals M = 3 once, bitwise"""
  from dynibar_amd import metrics
  c, tgt, *_ = exact(H, W, 'noisy')
  pred, t = dev_t(c['pred'], device), dev_t(tgt, device)
  ms = [dev_t(c['masks'][k], device) for k in ('fractional', 'dynamic', 'valid')]
  three = metrics.frame_sums(pred, t, ms, data_range=R, apply_valid=True)['sums'].cpu().numpy()
  for i, m in enumerate(ms):
    one = metrics.frame_sums(pred, t, [m], data_range=R, apply_valid=True)['sums'].cpu().numpy()
    assert_bits(one[0], three[i], f'mask {i} alone against the same mask among three')


def check_value_errors(device):
  """check 7: the ValueErrors of the Python layer"""
  import pytest
  from dynibar_amd import metrics
  a = torch.rand(9, 13, 3).to(device)
  m = torch.ones(9, 13, 3).to(device)
  with pytest.raises(ValueError, match='same dimensions'):
    metrics.calculate_ssim(a, a[:, :12], m)
  with pytest.raises(ValueError, match='same dimensions'):
    metrics.calculate_psnr(a, a[:8], m)
  with pytest.raises(ValueError, match='same dimensions'):
    metrics.nvidia_frame_metrics(a, a[:8], m)
  with pytest.raises(ValueError, match='7 x 7 window'):
    metrics.calculate_ssim(a[:6], a[:6], m[:6])
  with pytest.raises(ValueError, match='7 x 7 window'):
    metrics.structural_similarity(a[:, :6], a[:, :6], data_range=1.0)
  with pytest.raises(ValueError, match='float32'):
    metrics.calculate_psnr(a.double(), a.double(), m)
  with pytest.raises(ValueError, match='float32'):
    metrics.calculate_psnr(a, a, m.double())
  with pytest.raises(ValueError, match='float32'):
    metrics.calculate_ssim(a, (a * 255).to(torch.uint8), m)  # a uint8 target is nvidia_frame_metrics' alone
  with pytest.raises(ValueError, match='numpy array or a torch tensor'):
    metrics.calculate_psnr(a, a, 1.0)
  with pytest.raises(ValueError, match=r'must be \[9, 13, 3\]'):
    metrics.calculate_psnr(a, a, m[:8])
  with pytest.raises(ValueError, match='masks in one call'):
    metrics.frame_sums(a, a, [m] * 9, data_range=1.0)
  with pytest.raises(ValueError, match='masks in one call'):
    metrics.frame_sums(a, a, [], data_range=1.0)
  for bad in (0.0, -1.0, float('nan'), float('inf')):
    with pytest.raises(ValueError, match='data_range'):
      metrics.calculate_ssim(a, a, m, data_range=bad)
  with pytest.raises(ValueError, match='different devices|host or on a HIP device'):
    metrics.calculate_psnr(a, a, torch.ones(9, 13, 3, device='meta'))
  assert isinstance(metrics.nvidia_frame_metrics(a, (a * 255).to(torch.uint8), m[..., 0] > 0.5)['psnr'], float)  # uint8 target, bool [H, W] mask
