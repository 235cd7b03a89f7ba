"""The feature-encoder convolution kernels under the wave-level emulator on a tiny batch, against the real reference's feature maps."""
import os

import numpy as np
import pytest

import encoder_checks as E
import parity

pytestmark = pytest.mark.emu


def test_encoder(emu, golden_dir):
  E.assert_regime(emu, 'small', 2, 40, 56)  # on the emulator's 7 CUs: runs of several rows, one of them crossing from image 0 to image 1
  parity.check_encoder(emu, dict(np.load(os.path.join(golden_dir, 'encoder.npz'))), 'small')


def test_encoder_training_form(emu):
  """forward with saved activations + backward (im2col + training GEMM + InstanceNorm kernels) vs autograd through the oracle"""
  parity.check_encoder_training(emu, 'tiny')


# ---- the small twins of tests/test_gpu_encoder.py: on the emulator's 7 CUs thumbnails reach what the production shapes reach on 256 ----
def test_encoder_wavefront_switches_image(emu):
  """2 x 64 x 16: wavefronts that write tiles of image 0, flush its statistics, and go on with image 1 under the second coefficient table"""
  E.check_encoder_regime(emu, 'tall', calls=1)


def test_encoder_more_images_than_cus(emu):
  """9 x 16 x 16 on 7 CUs: grid = N, every workgroup exactly one image (the GPU suite's 300 x 16 x 16)"""
  E.check_encoder_regime(emu, 'nine', calls=1)


@pytest.mark.parametrize('name', ['odd', 'odd_w'])
def test_encoder_more_goldens(emu, golden_dir, name):
  """odd: 3 x 37 x 50, two image boundaries inside runs at both resolutions; odd_w: an odd width"""
  if name == 'odd':
    E.assert_regime(emu, 'odd', 3, 37, 50)
  parity.check_encoder(emu, dict(np.load(os.path.join(golden_dir, 'encoder_odd_w.npz' if name == 'odd_w' else 'encoder.npz'))), name)


def test_encoder_rejects_images_below_16(emu):
  E.check_encoder_rejects_small_images(emu)


@pytest.mark.parametrize('name', ['dim', 'const'])
def test_encoder_norm_statistics_conditioning(emu, name):
  E.check_encoder_conditioning(emu, name, shape=(2, 40, 56))


def test_im2col_and_its_adjoint(emu):
  for k, stride, C, H, W in E.im2col_cases(shapes=((16, 16), (19, 25))):
    E.check_im2col(emu, k, stride, C, H, W, N=1)
    if C == 64:
      E.check_col2im(emu, k, stride, H, W, N=1)


def test_instance_norm_kernels(emu):
  for HW in (1, 15, 16, 17, 255, 256, 257):
    for relu, with_res in ((False, False), (True, True)):
      E.check_instance_norm(emu, HW, 3 if HW == 17 else 1, relu, with_res)
  E.check_instance_norm_offset(emu, HW=1000, N=1)


def test_helper_argument_errors(emu):
  E.check_helper_argument_errors(emu)
