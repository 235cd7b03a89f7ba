"""Host-side checks of the logged view panels (dynibar_amd/view_log.py, csrc/dyn_viewlog.h): the yardstick itself -- the numpy restatements of
tests/view_log_cases.py against the REAL functions' outputs in tests/golden/view_log.npz, exactly -- the shipped colour tables, the percentile
plan, and the refusals that need no device."""
import numpy as np
import pytest
import torch

import view_log_cases as vc

G = vc.golden()


def test_fixture_records_its_versions_and_covers_the_cases():
  assert any(v.startswith('numpy 2.') for v in G['versions']) and any(v.startswith('matplotlib ') for v in G['versions'])
  for H, W in vc.GOLDEN_SHAPES:
    for name in vc.SCALAR_DATA:
      assert all(f'colorize/{name}/{H}x{W}/{k}' in G for k in ('x',) + vc.MAPS)
    for case in vc.FLOW_CASES:
      assert all(f'flow/{case}/{H}x{W}/{k}' in G for k in ('flow', 'img'))


@pytest.mark.skipif(int(np.__version__.split('.')[0]) < 2, reason='the contract is the arithmetic of numpy >= 2')
@pytest.mark.parametrize('H,W', vc.GOLDEN_SHAPES)
@pytest.mark.parametrize('name', vc.SCALAR_DATA)
def test_colorize_restatement_equals_the_real_function(H, W, name):
  x = G[f'colorize/{name}/{H}x{W}/x']
  for cmap in vc.MAPS:
    want = G[f'colorize/{name}/{H}x{W}/{cmap}']
    got = vc.colorize_restated(x, cmap)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape == (H, W, 3)
    assert np.array_equal(got, want), f'{name} {H}x{W} {cmap}: {(got != want).sum()} values differ'


@pytest.mark.skipif(int(np.__version__.split('.')[0]) < 2, reason='the contract is the arithmetic of numpy >= 2')
@pytest.mark.parametrize('H,W', vc.GOLDEN_SHAPES)
@pytest.mark.parametrize('case', vc.FLOW_CASES)
def test_flow_to_image_restatement_equals_the_real_function(H, W, case):
  f = G[f'flow/{case}/{H}x{W}/flow']
  before = f.copy()
  got, want = vc.flow_to_image_restated(f), G[f'flow/{case}/{H}x{W}/img']
  assert got.dtype == want.dtype == np.uint8 and np.array_equal(got, want), f'{case} {H}x{W}: {(got != want).sum()} bytes differ'
  assert np.array_equal(before, f, equal_nan=True)
  if case.endswith('unknown') or case == 'unknown_largest':
    unknown = (abs(f[..., 0]) > 200) | (abs(f[..., 1]) > 200)
    assert unknown.any() and not got[unknown].any()


def test_fma_chain_magnitude_equals_torch_norm():
  v, want = G['norm/v'], G['norm/mag']
  got = vc.magnitude(v)
  assert got.dtype == np.float32 and np.array_equal(got, want)
  assert np.array_equal(got, torch.norm(torch.from_numpy(v), dim=-1).numpy())
  plain = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
  assert (plain != want).any(), 'the vectors do not tell the fma chain from the plain sum'


def test_shipped_tables_equal_matplotlib():
  matplotlib = pytest.importorskip('matplotlib')
  from dynibar_amd import view_log
  assert view_log.MAPS == vc.MAPS
  for name in vc.MAPS:
    t = view_log.table(name)
    assert t.dtype == torch.float64 and tuple(t.shape) == (256, 3)
    assert np.array_equal(t.numpy(), matplotlib.colormaps[name](np.arange(256))[:, :3])


def test_product_does_not_import_matplotlib_or_cv2():
  import os
  import subprocess
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  code = ("import sys; import dynibar_amd.view_log as v; v.table('jet'); v.percentile_plan(100); "
          "assert 'matplotlib' not in sys.modules and 'cv2' not in sys.modules")
  subprocess.run([sys.executable, '-c', code], check=True, cwd=root)


@pytest.mark.parametrize('n', vc.PLAN_SIZES)
def test_percentile_plan_equals_numpy(n):
  from dynibar_amd import view_log
  rank, weight = view_log.percentile_plan(n)
  assert rank.dtype == np.int32 and rank.shape == (4,) and weight.dtype == np.float64 and weight.shape == (2,)
  assert bool(((rank >= 0) & (rank < n)).all()) and bool(((weight >= 0) & (weight <= 1)).all())
  rng = np.random.default_rng([n, 9])
  for x in (rng.standard_normal(n).astype(np.float32) ** 3, rng.choice(np.array([-1.0, 0.5, 2.0], dtype=np.float32), n),
            rng.random(n).astype(np.float32) * np.float32(1e-3) + np.float32(100.0)):
    want = np.percentile(x, (1, 99))
    got = vc.lerp_from_plan(x, rank, weight)
    assert want.dtype == np.float64 and np.array_equal(got, want), f'n={n}: {got.tolist()} vs {want.tolist()}'


def test_refusals_without_a_device():
  """host tensors are refused (no CPU fallback); the unknown map, the unbuilt options and the limits are refused before anything else"""
  from dynibar_amd import view_log
  x, f = torch.zeros(5, 6), torch.zeros(5, 6, 2)
  for call in (lambda: view_log.colorize(x), lambda: view_log.flow_to_image(f), lambda: view_log.ranges([x]), lambda: view_log.flow_max([f])):
    with pytest.raises(RuntimeError, match='HIP device'):  # (whether or not a device is present)
      call()
  with pytest.raises(ValueError, match="'jet' and 'gray'"):
    view_log.colorize(x, 'viridis')
  with pytest.raises(ValueError, match="'jet' and 'gray'"):
    view_log.table('hot')
  for kw in (dict(mask=x > 0), dict(range=(0.0, 1.0)), dict(append_cbar=True)):
    with pytest.raises(NotImplementedError):
      view_log.colorize(x, **kw)
  with pytest.raises(ValueError, match='1..4'):
    view_log.ranges([x] * 5)
  with pytest.raises(ValueError, match='1..12'):
    view_log.flow_max([f] * 13)
  with pytest.raises(ValueError, match='torch tensor'):
    view_log.colorize(np.zeros((5, 6), np.float32))
  with pytest.raises(ValueError, match='percentile'):
    view_log.percentile_plan(0)


def test_library_refuses_bad_arguments_on_the_host():
  """dyn_viewlog_* check their arguments in host code before anything is launched: with null pointers and no device they return DYN_E_INVALID"""
  from dynibar_amd import _lib
  lib = _lib.lib()
  assert lib.dyn_viewlog_ranges(0, 4, 4, None, None, None, None, None, None, None) == -1 and b'0 images' in lib.dyn_last_error()
  assert lib.dyn_viewlog_ranges(1, 4, 4, None, None, None, None, None, None, None) == -1 and b'required' in lib.dyn_last_error()
  assert lib.dyn_viewlog_flow_max(13, 4, 4, None, None, None) == -1 and b'13 flows' in lib.dyn_last_error()
  assert lib.dyn_viewlog_flow_max(1, 46341, 46341, None, None, None) == -1 and b'unsupported' in lib.dyn_last_error()
  assert lib.dyn_viewlog_panels(None, None) == -1 and b'null params' in lib.dyn_last_error()
  names = [lib.dyn_profile_name(i).decode() for i in range(lib.dyn_profile_count())]
  assert names[-3:] == ['k_viewlog_ranges', 'k_viewlog_flow_max', 'k_viewlog_panels']


def test_every_engine_build_exports_the_new_entry_points():
  import ctypes
  import os
  from dynibar_amd import _lib
  for name in _lib.ENGINE_LIBS:
    path = _lib.engine_path(name)
    assert os.path.exists(path), path
    dll = ctypes.CDLL(path)
    for fn in ('dyn_viewlog_ranges', 'dyn_viewlog_flow_max', 'dyn_viewlog_panels'):
      assert hasattr(dll, fn), f'{fn} is not exported by {os.path.basename(path)}'
