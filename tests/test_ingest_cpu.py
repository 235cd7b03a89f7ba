"""The restatements of the scene-preparation contracts (tests/ingest_cases.py) against an independent definition each, and the host parts of
dynibar_amd/ingest.py (the tables, the percentile plan, the pose and bounds assembly of the command-line tool).  No device."""
import numpy as np
import pytest
import torch

import ingest_cases as ic
from dynibar_amd import ingest


@pytest.mark.parametrize('Hs,Ws,Hd,Wd', ic.AREA_CPU_SHAPES)
@pytest.mark.parametrize('C', [1, 3])
def test_area_restatement_against_the_float64_box_average(Hs, Ws, Hd, Wd, C):
  src = ic.u8_image(Hs, Ws, C)
  got = ic.resize_area(src, (Wd, Hd)).astype(np.float64)
  avg = ic.box_average(src, (Wd, Hd))
  err = float(np.abs(got - avg).max())
  print(f'{Hs} x {Ws} -> {Hd} x {Wd}, C = {C}: max |out - avg| = {err:.4f}, bound {ic.area_bound(Hs, Ws, Hd, Wd):.4f}')
  assert err <= ic.area_bound(Hs, Ws, Hd, Wd)


def test_area_restatement_copy_and_constant():
  src = ic.u8_image(7, 9, 3)
  assert np.array_equal(ic.resize_area(src, (9, 7)), src)
  for Hs, Ws, Hd, Wd in ic.AREA_CPU_SHAPES:
    for v in (0, 1, 37, 254, 255):
      assert (ic.resize_area(np.full((Hs, Ws, 3), v, np.uint8), (Wd, Hd)) == v).all(), (Hs, Ws, v)


def test_area_two_by_two_ties_round_up_and_the_table_branch_to_even():
  """the cases the device tests use do hold ties: the 2 x 2 branch where (sum + 2) >> 2 and half-to-even part ways, the table branch where
  round-half-up and half-to-even part ways"""
  src = ic.u8_image(8, 12, 3)
  sums, block = ic.area_sums(src, (6, 4))
  assert block == (2, 2)
  assert int(np.sum((sums % 4 == 2) & ((sums >> 2) % 2 == 0))) > 0
  assert np.array_equal(ic.resize_area(np.array([[1, 1], [0, 0]], np.uint8), (1, 1)), [[1]])  # 0.5 -> 1
  assert np.array_equal(ic.resize_area(np.array([[3, 3], [2, 2]], np.uint8), (1, 1)), [[3]])  # 2.5 -> 3
  Hs, Ws, Hd, Wd, C = ic.AREA_TIE_CASE
  assert ic.table_ties(ic.u8_image(Hs, Ws, C, seed=ic.AREA_TIE_SEED), (Wd, Hd)) > 0


@pytest.mark.parametrize('s,d', [(15, 4), (23, 6), (1001, 1000), (1080, 288), (1920, 512), (46, 13), (9, 9)])
def test_area_tables_of_the_package_are_the_restatements(s, d):
  count, idx, w = ingest.area_table(s, d)
  tab = ic.decimation_table(s, d)
  assert w.dtype == np.float32 and idx.dtype == count.dtype == np.int32
  for i, row in enumerate(tab):
    assert count[i] == len(row)
    assert [(int(idx[i, k]), w[i, k]) for k in range(len(row))] == [(j, a) for j, a in row]
    assert abs(float(np.sum(w[i, :count[i]], dtype=np.float64)) - 1.0) < 2e-3 + 1e-6  # (the slivers the 1e-3 rule skips)
    assert all(0 <= j < s for j, _ in row)


@pytest.mark.parametrize('Hs,Ws,Hd,Wd', ic.LINEAR_SHAPES)
def test_linear_restatement_against_interpolate(Hs, Ws, Hd, Wd):
  src = ic.f32_image(Hs, Ws)
  got = ic.resize_linear(src, (Wd, Hd))
  exact = ic.resize_linear(src, (Wd, Hd), dtype=np.float64)
  other = torch.nn.functional.interpolate(torch.from_numpy(src)[None, None], size=(Hd, Wd), mode='bilinear', align_corners=False)[0, 0].numpy()
  own = float(np.abs(got - exact).max())
  limit = 2.0 * own + 2e-6 * float(np.abs(src).max())  # twice the restatement's own distance from the float64 evaluation + 2e-6 of the magnitude
  err = float(np.abs(other.astype(np.float64) - exact).max())
  print(f'{Hs} x {Ws} -> {Hd} x {Wd}: restatement {own:.2e}, F.interpolate {err:.2e} from the float64 evaluation, limit {limit:.2e}')
  assert got.dtype == np.float32 and err <= limit
  if (Hs, Ws) == (Hd, Wd):
    assert np.array_equal(got.view(np.uint32), src.view(np.uint32))


def test_nearest_restatement():
  assert ic.nearest_index(5, 7).tolist() == [0, 0, 1, 2, 2, 3, 4]
  for src in (ic.u8_image(5, 7), ic.u8_image(5, 7, 3), ic.f32_image(5, 7, 2)):
    assert np.array_equal(ic.resize_nearest(src, (7, 5)), src)
  m = np.array([[0, 1, 254, 255]], np.uint8)
  assert ic.resize_nearest(m, (4, 1), below=255).tolist() == [[1, 1, 1, 0]]
  assert np.array_equal(ic.resize_nearest(m, (4, 1), below=255), (1.0 - m.astype(np.float32) / 255.0 > 1e-3).astype(np.uint8))  # the loader's form
  allm = np.arange(256, dtype=np.uint8)[None]
  assert np.array_equal(ic.resize_nearest(allm, (256, 1), below=255), (1.0 - allm.astype(np.float32) / 255.0 > 1e-3).astype(np.uint8))


@pytest.mark.parametrize('H,W', ic.ERODE_SHAPES[:3] + [(35, 67)])
@pytest.mark.parametrize('r', ic.ERODE_RADII)
def test_erosion_restatement_against_scipy(H, W, r):
  from scipy import ndimage
  yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
  disk = (yy * yy + xx * xx) <= r * r
  for density in ic.DENSITIES:
    m = ic.mask01(H, W, density=density)
    want = ndimage.binary_erosion(m.astype(bool), structure=disk, border_value=1).astype(np.uint8)
    assert np.array_equal(ic.erode_disk(m, r), want), density


@pytest.mark.parametrize('n', ic.PLAN_SIZES)
def test_percentile_plan_against_numpy(n):
  x = ic.bounds_data('uniform', n)
  for q in (5, 95, 0, 100, 50, 37.5):  # a scalar q: float32 throughout
    rank, weight = ingest.percentile_plan(n, q)
    want = np.percentile(x, q)
    (got,) = ic.plan_percentile(x, rank, weight)
    assert weight.dtype == np.float32 and rank.shape == (1, 2)
    assert got.dtype == want.dtype == np.float32 and got.tobytes() == want.tobytes(), (n, q, got, want)
  rank, weight = ingest.percentile_plan(n, (5, 95))  # a sequence: float64
  want = np.percentile(x, (5, 95))
  got = np.array(ic.plan_percentile(x, rank, weight))
  assert got.dtype == want.dtype == np.float64 and got.tobytes() == want.tobytes()
  from dynibar_amd import view_log
  r1, w1 = view_log.percentile_plan(n)
  r2, w2 = ingest.percentile_plan(n, (1, 99))
  assert np.array_equal(r1, r2.reshape(4)) and np.array_equal(w1, w2)
  with pytest.raises(ValueError):
    ingest.percentile_plan(n, 101)
  with pytest.raises(ValueError):
    ingest.percentile_plan(0, 5)


def test_poses_bounds_rows_against_a_hand_built_case():
  """save_monocular_cameras.py:115-149: [-y, x, z | t | (h, w, f)] per frame, ravelled, then the frame's two bounds"""
  c2w = np.zeros((3, 4, 4))
  for i in range(3):
    c2w[i, :3, :4] = np.arange(12).reshape(3, 4) + 100 * i
    c2w[i, 3, 3] = 1
  bounds = np.array([[0.5, 9.0], [0.6, 8.0], [0.7, 7.0]], dtype=np.float32)
  rows = ingest.poses_bounds(c2w, bounds, 288, 512, 400.0, 402.0)
  assert rows.shape == (3, 17) and rows.dtype == np.float64
  for i in range(3):
    o = 100 * i
    # row r of the 3 x 5 matrix: columns 1, 0, -2, 3 of the rotation-translation block, then h / w / f
    want = [1 + o, 0 + o, -(2 + o), 3 + o, 288, 5 + o, 4 + o, -(6 + o), 7 + o, 512, 9 + o, 8 + o, -(10 + o), 11 + o, 401.0,
            float(bounds[i, 0]), float(bounds[i, 1])]
    assert rows[i].tolist() == want, i
  K = ingest.scaled_intrinsics(np.array([[800.0, 0, 0], [0, 802.0, 0], [960, 540, 1]]), 512, 288, 1920, 1080)
  assert np.allclose(K, [[800 * 512 / 1920, 0, 256], [0, 802 * 288 / 1080, 144], [0, 0, 1]])
  with pytest.raises(ValueError, match='fx'):
    ingest.scaled_intrinsics(np.array([[800.0, 0, 0], [0, 900.0, 0], [960, 540, 1]]), 512, 288, 1920, 1080)


def test_no_cpu_fallback():
  with pytest.raises((RuntimeError, ValueError), match='HIP device'):
    ingest.resize_area(ic.u8_image(6, 8, 3), (4, 3), device='cpu')
  with pytest.raises((RuntimeError, ValueError)):
    ingest.erode_disk(ic.mask01(5, 5), 1, device='cpu')
