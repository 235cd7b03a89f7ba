"""Checks of dynibar_amd.lpips shared by tests/emu/test_emu_lpips.py (the wave-level emulator) and tests/test_gpu_lpips.py (the MI355X).
The yardstick is tests/lpips_restatement.py; no limit is taken from the code under test.

The accuracy limit.  For tap l, ``rel_l`` is the largest ``max|d_l(fp32) - d_l(f64)| / max d_l(f64)`` over the whole pool of cases (shapes x
pairs x 2 seeds), both from the CPU restatement.  (Pooled: at 1 x 1 taps a single fp32 sample can land near zero error by luck.)  Every case
must have ``max|d_l(device) - d_l(f64)| <= 2 rel_l max d_l(f64)`` for every tap -- the project's convention, twice the fp32 reference's own
distance from float64 -- and ``|lpips - lpips_f64|`` under the all-ones mask no larger than the sum of those five allowances.
The masked sums are checked against longdouble sums of the device's own maps to 64 * 2^-53 relative: a term passes through fewer than 32
roundings on its way into a sum (the product, 6 butterfly steps and 2 additions in the workgroup, at most rows / 256 + 1 additions of rows,
2 and 6 more butterfly steps), the terms are non-negative.
"""
import functools

import numpy as np
import torch

import lpips_restatement as lr
import parity

EPS53 = 2.0 ** -53
SEEDS = (0, 1)


def bits(x):
  x = np.ascontiguousarray(x)
  return x.view(np.int32) if x.dtype == np.float32 else (x.view(np.int64) if x.dtype == np.float64 else x)


def assert_bits(got, want, what):
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, f'{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}'
  bad = bits(got) != bits(want)
  assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} elements differ in their bits, first at {tuple(np.argwhere(bad)[0])}'


def dev_t(x, device):
  return torch.from_numpy(np.ascontiguousarray(x)).to(device)


@functools.lru_cache(maxsize=None)
def reference(H, W, kind, seed):
  """the case, its numpy preparation and the restatement's maps in float64 and float32 (computed once, never changed)"""
  pred, tgt = lr.make_pair(H, W, kind, seed)
  x0, x1, valid = lr.prepare_scaled(pred, tgt)
  w = lr.random_weights(seed)
  d64, d32 = lr.maps(x0, x1, w, torch.float64), lr.maps(x0, x1, w, torch.float32)
  return dict(pred=pred, target=tgt, x0=x0, x1=x1, valid=valid, d64=d64, d32=d32)


@functools.lru_cache(maxsize=None)
def pool_rel(shapes):
  """rel_l over the pool shapes x pairs x seeds"""
  rel = [0.0] * 5
  for H, W in shapes:
    for kind in lr.PAIRS:
      for seed in SEEDS:
        r = reference(H, W, kind, seed)
        for l in range(5):
          rel[l] = max(rel[l], float(np.abs(r['d32'][l].astype(np.float64) - r['d64'][l]).max() / r['d64'][l].max()))
  print('  pooled rel_l of the float32 restatement over', shapes, ':', ' '.join(f'{v:.3e}' for v in rel))
  return tuple(rel)


_NETS = {}


def net_of(seed):
  from dynibar_amd import lpips
  if seed not in _NETS:
    _NETS[seed] = lpips.LPIPS(*lr.random_weights(seed))
  return _NETS[seed]


def run(device, H, W, kind, seed, mask_names=lr.MASKS, **kw):
  r = reference(H, W, kind, seed)
  ms = lr.make_masks(H, W, seed)
  out = net_of(seed).frame_sums(dev_t(r['pred'], device), dev_t(r['target'], device), [dev_t(ms[k], device) for k in mask_names], apply_valid=True, **kw)
  return r, ms, out


def check_preparation(device, H, W, kind):
  """check 1: the prepared, scaled images bit for bit, with and without the valid mask, from a uint8 and from a float32 target"""
  r, _, out = run(device, H, W, kind, 0, ('ones',), want_prepared=True)
  got = out['prepared'].cpu().numpy()
  assert_bits(got[0], r['x0'], f'lpips [{H}x{W} {kind}] prepared pred')
  assert_bits(got[1], r['x1'], f'lpips [{H}x{W} {kind}] prepared target')
  tf = r['target'].astype(np.float32) / np.float32(255)
  x0, x1, _ = lr.prepare_scaled(r['pred'], tf, apply_valid=False)
  raw = net_of(0).frame_sums(dev_t(r['pred'], device), dev_t(tf, device), [dev_t(lr.make_masks(H, W)['ones'], device)], want_prepared=True)
  got = raw['prepared'].cpu().numpy()
  assert_bits(got[0], x0, f'lpips [{H}x{W} {kind}] scaled pred, apply_valid off')
  assert_bits(got[1], x1, f'lpips [{H}x{W} {kind}] scaled float target, apply_valid off')
  if kind == 'border':
    assert (r['valid'] == 0).any() and not np.array_equal(x1, r['x1']), 'the valid mask must bite in this case'


def check_accuracy(device, H, W, kind, seed, shapes):
  """check 2"""
  rel = pool_rel(tuple(shapes))
  r, ms, out = run(device, H, W, kind, seed, ('ones',), want_maps=True)
  tag = f'lpips [{H}x{W} {kind} seed {seed}]'
  sizes = lr.tap_sizes(H, W)
  total = 0.0
  for l in range(5):
    d, ref = out['maps'][l].cpu().numpy(), r['d64'][l]
    assert d.dtype == np.float64 and d.shape == ref.shape == sizes[l], f'{tag} tap {l + 1}: map {d.shape}, restatement {ref.shape}, expected {sizes[l]}'
    allow = 2 * rel[l] * float(ref.max())
    err = float(np.abs(d - ref).max())
    total += allow
    print(f'  {tag} tap {l + 1} {d.shape}: max d {ref.max():.3e} device err {err:.3e} allowance {allow:.3e} (ratio to the fp32 pool {err / (allow / 2):.3f})')
    parity.record_margin(f'{tag} d_{l + 1} vs float64', err, allow)
    assert np.isfinite(d).all() and err <= allow, f'{tag} tap {l + 1}: device map off by {err:.3e}, allowance {allow:.3e}'
  from dynibar_amd import lpips
  got = lpips.lpips_of(out['sums'].cpu().tolist()[0])
  want = lr.masked_lpips(r['d64'], ms['ones'])
  print(f'  {tag}: lpips {got!r} float64 {want!r} err {abs(got - want):.3e} allowance {total:.3e}')
  parity.record_margin(f'{tag} lpips vs float64', abs(got - want), total)
  assert abs(got - want) <= total, f'{tag}: lpips {got!r} against {want!r} (allowance {total:.3e})'


def check_masks(device, H, W, kind):
  """check 3: six masks; sums against longdouble sums of the device's own maps, M_l exact, zero gives 0.0, ones the plain mean"""
  from dynibar_amd import lpips
  r, ms, out = run(device, H, W, kind, 0, want_maps=True)
  tag = f'lpips masks [{H}x{W} {kind}]'
  maps = [m.cpu().numpy() for m in out['maps']]
  sums = out['sums'].cpu().numpy()
  assert sums.shape == (6, 5, 2) and np.isfinite(sums).all()
  sizes = lr.tap_sizes(H, W)
  for i, k in enumerate(lr.MASKS):
    want = lr.masked_sums(maps, ms[k])
    for l in range(5):
      S, M = float(want[l][0]), float(want[l][1])
      lim = 64 * EPS53 * S
      parity.record_margin(f'{tag} {k} S_{l + 1}', abs(sums[i, l, 0] - S), max(lim, 1e-300))
      assert abs(sums[i, l, 0] - S) <= lim, f'{tag} {k} tap {l + 1}: S = {sums[i, l, 0]!r}, from the maps {S!r} (limit {lim:.3e})'
      assert sums[i, l, 1] == M, f'{tag} {k} tap {l + 1}: M = {sums[i, l, 1]!r}, exact {M!r}'
    got = lpips.lpips_of(sums[i].tolist())
    if k == 'zero':
      assert (sums[i] == 0).all() and got == 0.0
    if k == 'ones':
      assert [sums[i, l, 1] for l in range(5)] == [float(h * w) for h, w in sizes]
      mean = sum(float(m.astype(np.longdouble).mean()) for m in maps)
      assert abs(got - mean) <= 5 * 66 * EPS53 * mean, f'{tag}: ones gives {got!r}, the plain mean {mean!r}'
    if k == 'gap':  # empty at the last three taps' resolution, not at the first two: those taps contribute 0
      assert (sums[i, 2:] == 0).all() and (sums[i, :2, 1] > 0).all() and got == sums[i, 0, 0] / sums[i, 0, 1] + sums[i, 1, 0] / sums[i, 1, 1]
  if kind == 'border':  # valid_as_mask0: the valid mask of the preparation at every tap
    v = net_of(0).frame_sums(dev_t(r['pred'], device), dev_t(r['target'], device), (), apply_valid=True, valid_as_mask0=True)['sums'].cpu().numpy()
    want = lr.masked_sums(maps, r['valid'])
    for l in range(5):
      assert v[0, l, 1] == float(want[l][1]) and abs(v[0, l, 0] - float(want[l][0])) <= 64 * EPS53 * float(want[l][0]), f'{tag} valid as mask 0, tap {l + 1}'
    assert v[0, 0, 1] < sizes[0][0] * sizes[0][1]


def check_identical(device, H, W):
  """check 4: identical images give exactly 0.0 and every map is exactly 0 (float and uint8 targets of the same values differ: a float target)"""
  from dynibar_amd import lpips
  r = reference(H, W, 'noisy', 0)
  ms = lr.make_masks(H, W)
  p = dev_t(r['pred'], device)
  out = net_of(0).frame_sums(p, p.clone(), [dev_t(ms['ones'], device), dev_t(ms['fractional'], device)], apply_valid=True, want_maps=True)
  for l, m in enumerate(out['maps']):
    assert bool((m == 0).all()), f'lpips [{H}x{W}] identical images: map {l + 1} is not exactly 0'
  sums = out['sums'].cpu().numpy()
  assert (sums[:, :, 0] == 0).all() and (sums[:, :, 1] > 0).all()
  assert lpips.lpips_of(sums[0].tolist()) == 0.0 and net_of(0)(p, p.clone()) == 0.0


def check_independence(device, H, W):
  """check 5: M = 1, 3 and 8 give the same bits for a mask"""
  r = reference(H, W, 'noisy', 0)
  ms = lr.make_masks(H, W)
  p, t = dev_t(r['pred'], device), dev_t(r['target'], device)
  names = ('fractional', 'dynamic', 'ones', 'static', 'gap', 'zero', 'dynamic', 'fractional')
  eight = net_of(0).frame_sums(p, t, [dev_t(ms[k], device) for k in names], apply_valid=True)['sums'].cpu().numpy()
  three = net_of(0).frame_sums(p, t, [dev_t(ms[k], device) for k in names[3:6]], apply_valid=True)['sums'].cpu().numpy()
  assert_bits(three, eight[3:6], 'three masks against the same masks among eight')
  assert_bits(eight[0], eight[7], 'the same mask in two places of one call')
  for i in (0, 1, 4):
    one = net_of(0).frame_sums(p, t, [dev_t(ms[names[i]], device)], apply_valid=True)['sums'].cpu().numpy()
    assert_bits(one[0], eight[i], f'mask {names[i]} alone against the same mask among eight')
  v = net_of(0).frame_sums(p, t, [dev_t(ms['dynamic'], device)], apply_valid=True, valid_as_mask0=True)['sums'].cpu().numpy()
  assert_bits(v[1], eight[1], 'a mask behind valid_as_mask0 against the same mask among eight')


def check_inputs(device, H, W):
  """check 7, first part: numpy, host-tensor and device-tensor inputs give the same bits; [H, W], [H, W, 1], [H, W, 3] and bool masks"""
  from dynibar_amd import metrics
  r = reference(H, W, 'close', 0)
  ms = lr.make_masks(H, W)
  net = net_of(0)
  forms = dict(numpy=lambda x: x, host=lambda x: torch.from_numpy(x), device=lambda x: dev_t(x, device))
  res = {k: (net(f(r['pred']), f(r['target']), f(ms['dynamic'])), net(f(r['pred']), f(r['target'])),
             net(f(r['pred']), f(r['target'].astype(np.float32) / np.float32(255)), f(ms['fractional'])))
         for k, f in forms.items()}
  assert all(isinstance(v, float) for v in res['numpy'])
  assert res['host'] == res['numpy'] and res['device'] == res['numpy'], res
  dyn = ms['dynamic']
  alt = [net(r['pred'], r['target'], m) for m in (dyn[..., 0], np.tile(dyn, (1, 1, 3)), dyn[..., 0] > 0.5)]
  assert alt == [res['numpy'][0]] * 3, (alt, res['numpy'][0])
  want = lr.masked_lpips(r['d64'], ms['ones'])
  assert abs(res['numpy'][1] - want) <= 1e-3 * want  # (the accuracy is check 2's; this is the entry point's plumbing)
  # nvidia_frame_metrics with a network: the three new numbers are frame_sums' own, the old ones keep their bits
  old = metrics.nvidia_frame_metrics(dev_t(r['pred'], device), dev_t(r['target'], device), dev_t(dyn, device))
  new = metrics.nvidia_frame_metrics(dev_t(r['pred'], device), dev_t(r['target'], device), dev_t(dyn, device), lpips=net)
  assert set(new) == set(old) | {'lpips', 'dynamic_lpips', 'static_lpips'} and {k: new[k] for k in old} == old
  from dynibar_amd import lpips
  s = net.frame_sums(dev_t(r['pred'], device), dev_t(r['target'], device), [dev_t(dyn, device), dev_t(1 - dyn, device)], apply_valid=True,
                     valid_as_mask0=True)['sums'].cpu().tolist()
  assert [new['lpips'], new['dynamic_lpips'], new['static_lpips']] == [lpips.lpips_of(t) for t in s]
  assert all(isinstance(new[k], float) for k in ('lpips', 'dynamic_lpips', 'static_lpips')) and new['lpips'] > 0
  out = torch.full((2, 5, 2), -1.0, dtype=torch.float64).to(device)
  got = net.frame_sums(dev_t(r['pred'], device), dev_t(r['target'], device), [dev_t(dyn, device)], apply_valid=True, valid_as_mask0=True, out=out)
  assert got['sums'] is out and out.cpu().tolist() == s[:2]


def check_value_errors(device):
  """check 9: the ValueErrors of the device path"""
  import pytest
  from dynibar_amd import metrics
  net = net_of(0)
  a = torch.rand(33, 40, 3).to(device)
  m = torch.ones(33, 40, 1).to(device)
  for small in (a[:30], a[:, :30]):
    with pytest.raises(ValueError, match='31 x 31'):
      net.frame_sums(small, small, [torch.ones(small.shape[0], small.shape[1], 1).to(device)])
    with pytest.raises(ValueError, match='31 x 31'):
      net(small, small)
    with pytest.raises(ValueError, match='31 x 31'):
      metrics.nvidia_frame_metrics(small, small, torch.ones(small.shape[0], small.shape[1]).to(device), lpips=net)
  with pytest.raises(ValueError, match='same dimensions'):
    net(a, a[:32])
  with pytest.raises(ValueError, match='float32'):
    net(a.double(), a.double())
  with pytest.raises(ValueError, match='float32'):
    net.frame_sums(a.double(), a, [m])
  with pytest.raises(ValueError, match='float32 or uint8'):
    net.frame_sums(a, a.double(), [m])
  with pytest.raises(ValueError, match='float32 or bool'):
    net(a, a, m.double())
  with pytest.raises(ValueError, match=r'must be \[33, 40, 3\]'):
    net(a, a, m[:32])
  with pytest.raises(ValueError, match='masks in one call'):
    net.frame_sums(a, a, [m] * 9)
  with pytest.raises(ValueError, match='masks in one call'):
    net.frame_sums(a, a, [m] * 8, valid_as_mask0=True)
  with pytest.raises(ValueError, match='masks in one call'):
    net.frame_sums(a, a, [])
  with pytest.raises(ValueError, match='torch tensors'):
    net.frame_sums(a.cpu().numpy(), a, [m])
  with pytest.raises(ValueError, match='numpy array or a torch tensor'):
    net(a, a, 1.0)
  with pytest.raises(ValueError, match=r'out must be a contiguous float64 tensor \[1, 5, 2\]'):
    net.frame_sums(a, a, [m], out=torch.zeros(1, 5, 3, dtype=torch.float64).to(device))
  with pytest.raises(ValueError, match='different devices|host or on a HIP device'):
    net(a, a, torch.ones(33, 40, 1, device='meta'))
  assert net(a, (a * 255).to(torch.uint8), m[..., 0] > 0.5) >= 0.0  # uint8 target, bool [H, W] mask
