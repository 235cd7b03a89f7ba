"""The geometry / compositing / resampling kernels executed under the wave-level emulator, checked against the oracle.
This is a debugging aid for kernel indexing in a container without a GPU; the authoritative parity run is -m gpu."""
import os

import numpy as np
import pytest

import cases
import parity

pytestmark = pytest.mark.emu


def test_sampling(emu):
  parity.check_sampling(emu, 'small')


@pytest.mark.parametrize('name', ['small', 'harsh', 'noise'])
def test_project_gather(emu, name):
  parity.check_project_gather(emu, name)


def test_composite(emu):
  parity.check_composite(emu, R=9, S=64)
  parity.check_composite(emu, R=6, S=128, seed=1)


def test_fine_samples(emu, golden_dir):
  g = dict(np.load(os.path.join(golden_dir, 'stages_small.npz')))
  parity.check_fine_samples(emu, g)


def test_module_helper_exports(emu, golden_dir):
  g = dict(np.load(os.path.join(golden_dir, 'stages_small.npz')))
  parity.check_module_helpers(emu, g, 'small', with_fine=False)


@pytest.mark.parametrize('name', ['small', 'harsh', 'noise'])
def test_project_gather_same_matrix(emu, name):
  parity.check_project_gather_same_matrix(emu, name)


def test_projector_helper_methods(emu):
  print('  compute_angle max |err| vs oracle:', parity.check_projector_helpers(emu, 'small'))


def test_trajectory_points_fused_into_gather_and_flows(emu):
  parity.check_fused_trajectory(emu, 'small', S=16, R=3)
  parity.check_fused_trajectory(emu, 'kid', S=8, R=2, virtual_views=3)


def test_expected_scene_flow(emu):
  parity.check_expected_scene_flow(emu)


# ---- the per-ray kernels at their edges (small twins of tests/test_gpu_parity.py's entries) -----------------------------------------------
def test_sampling_edges(emu):
  parity.check_sampling_edges(emu, S=2)
  for R, S in ((3, 85), (4, 64), (1, 257)):  # R * S = 255, 256, 257: one element short of, exactly and one past a 256-thread workgroup
    parity.check_sampling_edges(emu, S=S, R=R)


def test_composite_edges(emu):
  parity.check_composite_edges(emu, shapes=[s for s in cases.COMPOSITE_SHAPES if s[0] < 100])


@pytest.mark.parametrize('R,S,N', cases.FINE_SAMPLE_SHAPES)
def test_fine_samples_edges(emu, R, S, N):
  r = parity.check_fine_samples_edges(emu, R, S, N, with_sample_pdf=(R, S, N) in cases.FINE_SAMPLE_PDF_SHAPES)
  print('  knot ties:', {k.split(' [')[0] + k[-7:-1]: v['knot_ties'] for k, v in r.items() if v['mismatches']}, ' largest excluded share:', max(v['excluded'] for v in r.values()))


@pytest.mark.parametrize('S,N', cases.RAMP_DETECTOR_SHAPES)
def test_ramp_detector(emu, S, N):
  parity.check_ramp_detector(emu, S, N)


def test_ramp_bits(emu):
  parity.check_ramp_bits(emu)


def test_project_gather_row_order_fallback(emu):
  parity.check_project_gather_row_order(emu)
