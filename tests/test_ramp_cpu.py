"""The deterministic u ramp of sample_pdf(det=True) (csrc/dyn_geometry.hip:linspace01), restated in NumPy, against torch.linspace -- and
the inputs of the ramp detector (tests/parity.py:check_ramp_detector) against what they claim.  No GPU, no emulator."""
import pytest
import torch

import cases
from oracle import ibr_oracle as O


def test_ramp_restatement_is_torch_linspace_for_every_sample_count():
  """n * step below N / 2, fma(-step, N - 1 - n, 1) from there on: the bits of torch.linspace(0, 1, N) on the CPU for N = 2 ... 512.  They belong
  to the torch build the goldens were made with (2.10, ATen kernels with fused multiply-add: AVX2 / AVX512); a build that rounds the product first
  gives the unfused form, which this test would report."""
  bad = [N for N in range(2, 513) if not torch.equal(cases.linspace01_restated(N), torch.linspace(0.0, 1.0, N))]
  assert not bad, f'restated ramp != torch.linspace for N = {bad[:20]} ({len(bad)} sample counts)'


def test_unfused_ramp_differs_at_the_recorded_positions():
  """the formula the kernels had before (product rounded to fp32, then subtracted): one ulp off in the upper half -- the positions recorded for
  N = 64, and none for N = 2, 3, 17, 32, 65.  Keeps the restatement above honest: it can tell the two apart."""
  ref = torch.linspace(0.0, 1.0, 64)
  assert torch.nonzero(cases.linspace01_restated(64, fused=False) != ref).flatten().tolist() == [41, 43, 45, 48, 50]
  for N, n_diff in ((2, 0), (3, 0), (17, 0), (32, 0), (65, 0), (128, 9), (255, 20), (256, 23)):
    assert int((cases.linspace01_restated(N, fused=False) != torch.linspace(0.0, 1.0, N)).sum()) == n_diff, N


@pytest.mark.parametrize('S,N', cases.RAMP_DETECTOR_SHAPES)
def test_ramp_detector_inputs(S, N):
  """uniform weights: the kernel's cdf recipe (restated) gives torch's cdf bit for bit, at least every second ramp value is a knot, and the
  unfused ramp would move an index at (128, 64) and (256, 128) -- so the detector can fail"""
  ww = torch.zeros(3, S - 2)
  cdf = O.pdf_to_cdf(ww)
  assert torch.equal(cases.kernel_cdf_restated(ww), cdf)
  u = torch.linspace(0.0, 1.0, N)
  assert int((u[:, None] == cdf[0][None, :]).any(-1).sum()) >= N // 2
  bins = torch.arange(S - 1, dtype=torch.float32)[None].repeat(3, 1)
  inds = O.invert_cdf(bins, cdf, u[None].repeat(3, 1))[1]
  inds_unfused = O.invert_cdf(bins, cdf, cases.linspace01_restated(N, fused=False)[None].repeat(3, 1))[1]
  flips = int((inds != inds_unfused).sum()) // 3
  print(f'  S={S} N={N}: the unfused ramp flips {flips} of {N} indices per ray')
  if (S, N) != (64, 32):
    assert flips > 0
