"""CPU-side checks of the LPIPS path (dynibar_amd/lpips.py, csrc/dyn_lpips.h): the restatement the device is held to (tests/lpips_restatement.py)
against independent torch forms, the state-dict mapping and every ValueError of ``LPIPS(...)``, the host-side packing and argument checks of the
C entry points, and the unchanged outputs of the evaluation without ``lpips=``.  The kernels themselves: tests/test_gpu_lpips.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import lpips_restatement as lr
from dynibar_amd import _lib, lpips, metrics, nvidia_eval


def test_integer_nearest_rule_equals_interpolate():
  """src = (dst * n_in) // n_out is F.interpolate(mode='nearest') at all four shapes and five taps"""
  for H, W in lr.SHAPES:
    m = torch.arange(H * W, dtype=torch.float32).view(1, 1, H, W)
    for h, w in lr.tap_sizes(H, W):
      want = F.interpolate(m, size=(h, w), mode='nearest')[0, 0].numpy()
      got = lr.resize_mask(m[0, 0].numpy(), h, w)
      assert np.array_equal(got, want.astype(np.float64)), (H, W, h, w)
  assert lr.tap_sizes(288, 512) == ((71, 127), (35, 63), (17, 31), (17, 31), (17, 31)) == lpips.tap_sizes(288, 512)
  assert lr.tap_sizes(31, 31) == ((7, 7), (3, 3), (1, 1), (1, 1), (1, 1)) and lr.tap_sizes(32, 45)[:3] == ((7, 10), (3, 4), (1, 1))
  assert lr.tap_sizes(67, 95)[:3] == ((16, 23), (7, 11), (3, 5))
  for H, W in lr.SHAPES:
    assert lpips.tap_sizes(H, W) == lr.tap_sizes(H, W)


def test_all_ones_mask_is_the_plain_mean_and_empty_taps_contribute_nothing():
  H, W = 67, 95
  pred, tgt = lr.make_pair(H, W, 'noisy')
  x0, x1, _ = lr.prepare_scaled(pred, tgt)
  ds = lr.maps(x0, x1, lr.random_weights(0), torch.float64)
  ms = lr.make_masks(H, W)
  plain = sum(float(d.mean()) for d in ds)
  assert abs(lr.masked_lpips(ds, ms['ones']) - plain) <= 1e-14 * plain and plain > 1e-3
  assert lr.masked_lpips(ds, ms['zero']) == 0.0
  gap = lr.masked_sums(ds, ms['gap'])
  assert all(m == 0 for _, m in gap[2:]) and all(m > 0 for _, m in gap[:2])
  assert lpips.lpips_of([(1.0, 4.0), (0.0, 0.0), (3.0, 2.0), (0.0, 0.0), (0.0, 1.0)]) == 0.25 + 1.5
  assert all(float(d.max()) > 1e-5 for d in ds), 'taps of order 1e-3 to 1e-2 with these weights'


def test_restatement_taps_equal_a_sequential_alexnet():
  """torchvision's layout written out as nn.Sequential with the same weights: the taps after each ReLU, an independent check of indices and pooling"""
  alex, _ = lr.random_weights(0)
  seq = nn.Sequential(nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(), nn.MaxPool2d(3, 2), nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(), nn.MaxPool2d(3, 2),
                      nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(), nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(), nn.Conv2d(256, 256, 3, padding=1),
                      nn.ReLU()).double()
  seq.load_state_dict({k.replace('features.', ''): v.double() for k, v in alex.items()})
  for H, W in ((31, 31), (67, 95)):
    x = torch.rand(2, 3, H, W, dtype=torch.float64) * 4 - 2
    want, y = [], x
    with torch.no_grad():
      for i, layer in enumerate(seq):
        y = layer(y)
        if i in (1, 4, 7, 9, 11):
          want.append(y)
      got = lr.features(x, alex, torch.float64)
    assert [tuple(t.shape[2:]) for t in got] == list(lr.tap_sizes(H, W)) and [t.shape[1] for t in got] == list(lr.CHANNELS)
    for g, w in zip(got, want):
      assert torch.equal(g, w)


def test_preparation_is_im2tensor_and_the_scaling_layer():
  pred, tgt = lr.make_pair(31, 31, 'border')
  x0, x1, valid = lr.prepare_scaled(pred, tgt)
  assert x0.dtype == x1.dtype == np.float32 and (valid == 0).any()
  a = pred * valid[..., None]
  want = ((a / np.float32(0.5) - np.float32(1)) - np.array([-.030, -.088, -.188], np.float32)) / np.array([.458, .448, .450], np.float32)
  assert np.array_equal(x0, want)
  assert np.allclose(x0[valid == 0], (np.float32(-1) - lr.SHIFT) / lr.SCALE)


def _dicts():
  alex, lin = lr.random_weights(0)
  return dict(alex), dict(lin)


def test_state_dict_mapping_and_value_errors():
  alex, lin = _dicts()
  full = dict(alex)
  full['classifier.1.weight'] = torch.zeros(4, 4)  # torchvision's further keys are ignored
  net = lpips.LPIPS(full, lin)
  assert [a.size for a in net._arrs] == [64 * 363, 64, 192 * 1600, 192, 384 * 1728, 384, 256 * 3456, 256, 256 * 2304, 256, 64, 192, 384, 256, 256]
  assert np.array_equal(net._arrs[2], alex['features.3.weight'].numpy().reshape(-1)) and np.array_equal(net._arrs[12], lin['lin2.model.1.weight'].numpy().reshape(-1))
  lpips.LPIPS({k: v.double().numpy() for k, v in alex.items()}, lin)  # numpy arrays and other float types are converted
  for key in ('features.0.weight', 'features.10.bias'):
    with pytest.raises(ValueError, match=f'no {key!r}'):
      lpips.LPIPS({k: v for k, v in alex.items() if k != key}, lin)
  with pytest.raises(ValueError, match="no 'lin3.model.1.weight'"):
    lpips.LPIPS(alex, {k: v for k, v in lin.items() if k != 'lin3.model.1.weight'})
  with pytest.raises(ValueError, match=r'features.3.weight has shape \(192, 64, 3, 3\)'):
    lpips.LPIPS({**alex, 'features.3.weight': alex['features.3.weight'][:, :, :3, :3]}, lin)
  with pytest.raises(ValueError, match=r'features.6.bias has shape'):
    lpips.LPIPS({**alex, 'features.6.bias': alex['features.6.bias'][:-1]}, lin)
  with pytest.raises(ValueError, match=r'lin1.model.1.weight has shape \(192,\)'):
    lpips.LPIPS(alex, {**lin, 'lin1.model.1.weight': lin['lin1.model.1.weight'].reshape(-1)})
  neg = lin['lin4.model.1.weight'].clone()
  neg[0, 7] = -1e-6
  with pytest.raises(ValueError, match='lin4.model.1.weight has a negative weight'):
    lpips.LPIPS(alex, {**lin, 'lin4.model.1.weight': neg})
  for bad in (float('inf'), float('nan')):  # out of range for the fp32 engine: anything that is not finite
    w = alex['features.8.weight'].clone()
    w[3, 2, 1, 0] = bad
    with pytest.raises(ValueError, match='features.8.weight has an element that is not finite'):
      lpips.LPIPS({**alex, 'features.8.weight': w}, lin)
  with pytest.raises(ValueError, match='floating-point'):
    lpips.LPIPS({**alex, 'features.0.bias': torch.zeros(64, dtype=torch.int64)}, lin)


def test_input_value_errors_come_before_any_device_work():
  net = lpips.LPIPS(*_dicts())
  a = torch.rand(33, 40, 3)
  m = torch.ones(33, 40, 1)
  for small in (a[:30], a[:, :30]):
    with pytest.raises(ValueError, match='31 x 31'):
      net.frame_sums(small, small, [m])
    with pytest.raises(ValueError, match='31 x 31'):
      net(small.numpy(), small.numpy())
  with pytest.raises(ValueError, match='pred must be float32'):
    net.frame_sums(a.double(), a, [m])
  with pytest.raises(ValueError, match='pred must be float32'):
    net.frame_sums(a[..., :2], a[..., :2], [m])
  with pytest.raises(ValueError, match='target must be float32 or uint8'):
    net.frame_sums(a, a.to(torch.int32), [m])
  with pytest.raises(ValueError, match='target must be float32 or uint8'):
    net.frame_sums(a, a[:32], [m])
  with pytest.raises(ValueError, match='same dimensions'):
    net(a, a[:32])
  with pytest.raises(ValueError, match='torch tensors'):
    net.frame_sums(a.numpy(), a, [m])


def test_no_cpu_fallback():
  net = lpips.LPIPS(*_dicts())
  a = np.full((33, 40, 3), 0.5, np.float32)
  if torch.cuda.is_available():
    assert net(a, a) == 0.0
    return
  with pytest.raises(RuntimeError, match='HIP device'):
    net(a, a)
  with pytest.raises(RuntimeError, match='HIP device'):
    metrics.nvidia_frame_metrics(a, a, a, lpips=net)


def test_symbols_struct_and_profile_names():
  lib = _lib.lib()
  for name in ('dyn_lpips_blob_floats', 'dyn_lpips_pack', 'dyn_lpips_workspace_bytes', 'dyn_lpips_map_doubles', 'dyn_lpips_frame'):
    assert hasattr(lib, name) and name in _lib._FUNC_SPECS
  fields = dict(_lib._STRUCT_SPECS['DynLpipsParams'])
  assert fields['maps'] is ctypes.c_void_p and fields['workspace_bytes'] is ctypes.c_size_t and fields['mask_stride'] is ctypes.c_long
  names = [lib.dyn_profile_name(i).decode() for i in range(lib.dyn_profile_count())]
  for k in ('k_lpips_prep', 'k_lpips_conv', 'k_lpips_pool', 'k_lpips_tap', 'k_lpips_sums', 'k_lpips_finish'):
    assert k in names


def test_packing_runs_on_the_host_and_validates():
  lib = _lib.lib()
  net = lpips.LPIPS(*_dicts())
  blob = net._blob(torch.device('cpu')).numpy()
  n = lib.dyn_lpips_blob_floats()
  assert blob.shape == (n,) and np.isfinite(blob).all()
  # every weight, bias and lin value is in the blob exactly once (the rest is the zero padding of K)
  total = sum(float(np.abs(a.astype(np.float64)).sum()) for a in net._arrs)
  assert abs(float(np.abs(blob.astype(np.float64)).sum()) - total) <= 1e-9 * total
  assert np.count_nonzero(blob) == sum(int(np.count_nonzero(a)) for a in net._arrs)
  assert np.array_equal(blob[-256:], net._arrs[14]) and np.array_equal(blob[-(64 + 192 + 384 + 256 + 256):][:64], net._arrs[10])
  # the C packer's own checks (the Python layer refuses these earlier)
  err = lambda: lib.dyn_last_error().decode()
  ptrs = lambda arrs: (ctypes.c_void_p * 15)(*[a.ctypes.data if a is not None else None for a in arrs])
  out = np.zeros(n, np.float32)
  assert lib.dyn_lpips_pack(ptrs(net._arrs), out.ctypes.data, n - 1) == -1 and 'blob too small' in err()
  assert lib.dyn_lpips_pack(ptrs(net._arrs[:4] + [None] + net._arrs[5:]), out.ctypes.data, n) == -1 and 'tensor 4 is NULL' in err()
  assert lib.dyn_lpips_pack(None, out.ctypes.data, n) == -1 and 'null pointer' in err()
  bad = [a.copy() for a in net._arrs]
  bad[11][5] = -0.5
  assert lib.dyn_lpips_pack(ptrs(bad), out.ctypes.data, n) == -1 and 'lin1 has a negative' in err()
  bad = [a.copy() for a in net._arrs]
  bad[6][100] = np.inf
  assert lib.dyn_lpips_pack(ptrs(bad), out.ctypes.data, n) == -1 and 'features weight 3' in err()
  assert lib.dyn_lpips_pack(ptrs(net._arrs), out.ctypes.data, n) == 0 and np.array_equal(out, blob)


def _params(**kw):
  base = dict(H=31, W=40, M=1, blob=16, pred=8, target=8, masks=8, mask_stride=31 * 40 * 3, mask_channels=3, workspace=16, workspace_bytes=1 << 30)
  base.update(kw)
  return _lib.params('DynLpipsParams', **base)


def test_argument_errors_without_a_device():
  lib = _lib.lib()
  err = lambda: lib.dyn_last_error().decode()
  assert lib.dyn_lpips_frame(None, 8, None) == -1 and 'dyn_lpips_frame: null params' in err()
  for kw, msg in ((dict(H=30), '31 x 31'), (dict(W=30), '31 x 31'), (dict(H=1 << 15, W=1 << 15), 'too large'), (dict(M=0), 'M=0 masks'), (dict(M=9), 'M=9 masks'),
                  (dict(blob=None), 'are required'), (dict(pred=None), 'are required'), (dict(target=None), 'are required'),
                  (dict(masks=None), 'masks is required'), (dict(mask_channels=2), 'mask_channels=2'), (dict(M=2, mask_stride=10), 'mask_stride'),
                  (dict(workspace=None), 'workspace'), (dict(workspace_bytes=16), 'workspace of 16 bytes'), (dict(workspace=24), '16-byte aligned'),
                  (dict(blob=8), '16-byte aligned'), (dict(maps=12), '8-byte aligned')):
    assert lib.dyn_lpips_frame(_params(**kw), 8, None) == -1, kw
    assert msg in err(), (kw, err())
  assert lib.dyn_lpips_frame(_params(), None, None) == -1 and 'are required' in err()
  assert lib.dyn_lpips_frame(_params(), 12, None) == -1 and '8-byte aligned' in err()
  assert lib.dyn_lpips_frame(_params(masks=None, valid_as_mask0=1, workspace_bytes=0), 8, None) == -1 and 'workspace of 0 bytes' in err()


def test_workspace_and_map_sizes():
  lib = _lib.lib()
  f, g = lib.dyn_lpips_workspace_bytes, lib.dyn_lpips_map_doubles
  assert f(30, 40, 1) == 0 and f(40, 30, 1) == 0 and f(31, 31, 0) == 0 and f(31, 31, 9) == 0 and f(1 << 15, 1 << 15, 1) == 0 and f(-1, 40, 1) == 0
  assert g(30, 40) == 0 and g(31, 31) == 49 + 9 + 3
  for H, W in lr.SHAPES:
    assert g(H, W) == sum(h * w for h, w in lr.tap_sizes(H, W))
    assert f(H, W, 1) > 0 and f(H, W, 1) % 16 == 0 and f(H, W, 8) >= f(H, W, 1)
  sizes = [f(h, w, 3) for h, w in lr.SHAPES]
  assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[-1] < 64 << 20


def test_the_evaluation_without_a_network_is_unchanged():
  assert nvidia_eval.NUMBERS == ('psnr', 'ssim', 'dynamic_psnr', 'dynamic_ssim', 'static_psnr', 'static_ssim')
  assert nvidia_eval.LPIPS_NUMBERS == ('lpips', 'dynamic_lpips', 'static_lpips')
  rows = [[3.0, 20.0, 30.0], [1.0, 5.0, 10.0], [0.0, 7.0, 8.0]]
  old = nvidia_eval.numbers_of(rows, 2, 5)
  assert set(old) == set(nvidia_eval.NUMBERS) | {'valid_fraction'} and old['static_psnr'] == 0 and old['valid_fraction'] == 1.0
  taps = [[[1.0, 2.0]] * 5, [[0.0, 0.0]] * 5, [[3.0, 4.0], [0.0, 0.0], [1.0, 8.0], [0.0, 1.0], [0.0, 0.0]]]
  new = nvidia_eval.numbers_of(rows, 2, 5, taps)
  assert {k: new[k] for k in old} == old and set(new) == set(old) | set(nvidia_eval.LPIPS_NUMBERS)
  assert (new['lpips'], new['dynamic_lpips'], new['static_lpips']) == (2.5, 0.0, 0.875)
  import inspect
  for fn in (nvidia_eval.views, nvidia_eval.evaluate, metrics.nvidia_frame_metrics):
    assert inspect.signature(fn).parameters['lpips'].default is None
