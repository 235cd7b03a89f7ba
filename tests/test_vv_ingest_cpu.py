"""Host-side checks of the float INTER_AREA restatement (tests/vv_ingest_cases.py) and of the pose algebra of ingest.build_virtual_views:
no GPU."""
import numpy as np
import pytest

import ingest_cases as ic
import vv_ingest_cases as vc


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('Hs,Ws,Hd,Wd', vc.AREA_F32_CASES)
def test_restatement_against_its_float64_evaluation(Hs, Ws, Hd, Wd, C):
  """The fp32 restatement against the same weighted average with the same fp32 coefficients in double.  For a pixel with n_x, n_y taps the
  bound is (n_x + n_y + 2) * 2^-23 * max|src|: one rounding of at most 2^-24 relative per coefficient, product and add, doubled to cover the
  second-order terms.  Derived, not measured."""
  src = vc.f01_image(Hs, Ws, C, seed=1)
  got = vc.resize_area_f32(src, (Wd, Hd))
  exact = vc.resize_area_f32(src, (Wd, Hd), dtype=np.float64)
  assert got.dtype == np.float32 and exact.dtype == np.float64 and got.shape == exact.shape == (Hd, Wd, C)
  ny, nx = vc.area_taps(Hs, Ws, Hd, Wd)
  bound = (nx[None, :, None] + ny[:, None, None] + 2) * 2.0 ** -23 * float(np.abs(src).max())
  err = np.abs(got.astype(np.float64) - exact)
  print(f'{Hs} x {Ws} -> {Hd} x {Wd} x {C} ({vc.area_branch(Hs, Ws, Hd, Wd)}): worst error {(err / bound).max():.3f} of the bound')
  assert (err <= bound).all()


def test_branches_of_the_cases():
  assert [vc.area_branch(*s) for s in vc.AREA_F32_CASES] == ['table', 'block', 'block', 'table', 'block', 'enlarge', 'enlarge']


def test_equal_sizes_are_the_identity():
  src = vc.f01_image(7, 9, 3)
  assert vc.resize_area_f32(src, (9, 7)).tobytes() == src.tobytes()


def test_enlarging_weights():
  """area semantics: a destination pixel is the average of the source over the cell it covers.  Doubling: every cell lies in one source
  pixel, so the pixels are replicated; 2 -> 3: the middle cell covers half of each source pixel"""
  s0, f = vc.enlarge_axis(4, 8)
  assert s0.tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and f.tolist() == [0] * 8
  src = np.arange(4, dtype=np.float32).reshape(1, 4, 1)
  assert vc.resize_area_f32(src, (8, 1))[0, :, 0].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
  s0, f = vc.enlarge_axis(2, 3)
  assert s0.tolist() == [0, 0, 1] and f.tolist() == [0, 0.5, 0]
  assert vc.resize_area_f32(src[:, :2], (3, 1))[0, :, 0].tolist() == [0, 0.5, 1]
  flat = np.full((5, 7, 2), 0.375, np.float32)  # the weights of a pixel sum to 1
  for size in ((12, 9), (12, 3)):  # both axes enlarge; one shrinks
    assert np.allclose(vc.resize_area_f32(flat, size), 0.375, rtol=3e-7, atol=0)


def test_block_sum_order_is_the_scalar_loops():
  """3 x 2: sum = 0 + (((S0 + S1) + S2) + S3), then + S4, + S5; times fp32 1 / 6"""
  src = vc.f01_image(2, 3, 1, seed=2)
  s = src.reshape(-1)
  want = ((((np.float32(0) + (((s[0] + s[1]) + s[2]) + s[3])) + s[4]) + s[5]) * (np.float32(1) / np.float32(6)))
  assert vc.resize_area_f32(src, (1, 1)).reshape(-1)[0].tobytes() == np.float32(want).tobytes()


def test_relative_transforms_are_frame_batchs():
  from dynibar_amd import ingest
  img, disp, K, c2w, vsv = vc.vv_inputs()
  rot, tr = ingest.relative_transforms(c2w, vsv)
  assert rot.shape == (3, 8, 3, 3) and tr.shape == (3, 8, 3) and rot.dtype == np.float64
  for f in (0, 2):
    for v in (0, 7):
      tgt = np.eye(4)
      tgt[:3, :4] = vsv[f, v]
      T = np.linalg.inv(tgt) @ c2w[f]
      assert np.array_equal(rot[f, v], T[:3, :3]) and np.array_equal(tr[f, v], T[:3, 3])
  # the poses of the shared inputs move every view by a few pixels at most: 63 * bound / depth = 4 px at the nearest pixel
  assert 0 < np.abs(tr).max() * K[0, 0] * float(disp.max()) < 6.0


def test_relative_transforms_against_the_inverse_written_out():
  """ingest.relative_transforms and virtual_views.frame_batch share one statement of the pose algebra; this one is the test's own:
  inv([vv_c2w; 0 0 0 1]) @ c2w in float64 for every frame and view, exact.  float32 poses are promoted before the product, not after."""
  from dynibar_amd import ingest
  _, _, _, c2w, vsv = vc.vv_inputs()
  c2w = c2w.copy()
  c2w[:, :3, :3] = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])  # a rotation, so that every entry of the product matters
  for ref in (c2w, c2w.astype(np.float32)):
    rot, tr = ingest.relative_transforms(ref, vsv)
    assert rot.dtype == tr.dtype == np.float64
    for f in range(3):
      for v in range(8):
        tgt = np.concatenate([vsv[f, v].astype(np.float64), [[0.0, 0.0, 0.0, 1.0]]])
        T = np.linalg.inv(tgt) @ ref[f].astype(np.float64)
        assert np.array_equal(rot[f, v], T[:3, :3]) and np.array_equal(tr[f, v], T[:3, 3]), (f, v)
  assert np.abs(rot[0, 0] - np.eye(3)).max() > 0.3

