"""The training kernels (csrc/dyn_train.hip, the gather backward) under the wave-level emulator: a tiny static bootstrap step, values and
every gradient against autograd through the oracle.  Debugging aid in a container without a GPU; -m gpu is authoritative."""
import os

import pytest
import torch

import parity

pytestmark = pytest.mark.emu


def test_train_gemm_modes(emu):
  parity.check_train_gemm(emu)


def test_train_gemm_random_shapes(emu):
  parity.check_train_gemm_fuzz(emu, n_cases=9, max_rows=400)


def test_train_composite(emu):
  parity.check_train_composite(emu, lengths=(5, 64, 100), R=3)


def test_train_attention(emu):
  parity.check_train_attention(emu, lengths=(5, 16, 37, 120), R=2)


def test_static_bootstrap_step(emu):
  parity.check_train_static(emu, 'few', S=8, R=2)


def test_static_bootstrap_step_three_views(emu):
  """3 static source views: the moments of the training embed kernel follow the reference's torch.cross over the view axis (csrc/dyn_device.h)."""
  parity.check_train_static(emu, 'cross_views', S=8, R=2)


def test_static_bootstrap_step_kid_config(emu):
  parity.check_train_static(emu, 'few', S=8, R=2, aa=False, mask_rgb=True)


def test_dual_branch_step(emu):
  """second slice: DynibarDynamic + raw2outputs, gradients to both nets and both feature-map sets"""
  parity.check_train_dual(emu, 'few', S=8, R=2)


# the motion path's autograd Functions (dynibar_amd/train_motion.py) one by one, every dispatch variant of their backward kernels
@pytest.mark.parametrize('kw', [dict(name='few', S=16), dict(name='harsh', S=4), dict(name='few', S=8, F=16), dict(name='harsh', S=8, maps=False)],
                         ids=['F32-ray', 'F32-short-rays-outside', 'F16', 'xyz-only'])
def test_gather_function(emu, kw):
  """GatherFunction w.r.t. the feature maps and the displaced points: k_gather_bwd32_ray / k_gather_bwd32 / k_gather_bwd, k_gather_bwd_pts32 /
  k_gather_bwd_pts; taps outside the image and behind a camera; the points alone requiring grad"""
  parity.check_gather_fn(emu, **kw)


@pytest.mark.parametrize('kw', [dict(B=6), dict(B=10, ref=22, offsets=(-2, -1, 0, 1, 2, 3))], ids=['B6', 'B10'])
def test_trajectory_function(emu, kw):
  """TrajectoryFunction: k_trajectory_bwd8 (B <= 8) and k_trajectory_bwd; rows wrapping modulo the frame count, virtual-view rows of -1"""
  parity.check_trajectory_fn(emu, **kw)


@pytest.mark.parametrize('S,R,V', [(1, 5, 1), (63, 5, 16), (64, 5, 16), (65, 7, 1), (200, 5, 16)])
def test_render_flows_function(emu, S, R, V):
  """RenderFlowsFunction: d weights and d displaced points, rays shorter than, as long as and longer than one wavefront of samples"""
  parity.check_render_flows_fn(emu, S=S, R=R, V=V)


@pytest.mark.parametrize('S,div', [(4, 1.0), (16, 2.5)])
def test_motion_mlp_function(emu, S, div):
  """MotionMLPFunction: every parameter and the points; S = 4 (n_last rounds to 0: every sample zeroed) and sf_mag_div != 1"""
  parity.check_motion_mlp_fn(emu, S=S, sf_mag_div=div)


@pytest.mark.skipif(not os.environ.get('DYN_EMU_FULL'), reason='17 minutes under the emulator: set DYN_EMU_FULL=1 (the -m gpu suite runs the same check on hardware)')
def test_full_training_iteration(emu, golden_dir):
  """third slice: render_rays_mono(is_train=True) under grad mode, the reference's main-loop loss, every gradient incl. MotionMLP and the
  trajectory basis against the real reference's autograd digests"""
  import os
  import numpy as np
  parity.check_train_mono(emu, dict(np.load(os.path.join(golden_dir, 'mono_train_grad.npz'))), losses=('full', 'flow', 'cycle'))
