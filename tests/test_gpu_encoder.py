"""-m gpu tests of the feature encoder at the shapes it runs in production and at the edges of its work split (tests/encoder_checks.py):
every reference is the oracle's encoder in float64 on the CPU."""
import os
import subprocess
import sys

import pytest
import torch

import encoder_checks as E
import parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'the -m gpu tests need an MI355X'
  from dynibar_amd import _lib
  _lib.lib()
  return 'cuda:0'


@pytest.mark.parametrize('name', ['eval', 'train', 'ragged', 'just_over', 'many', 'min'])
def test_encoder_work_split_regimes(dev, name):
  """k_enc_conv where a workgroup walks several output rows, crosses an image boundary (second coefficient table, flush of the statistics at the
  switch), where there are more images than CUs, and at odd sizes with 1 to 25 live lanes in a row's last tile; the regime is asserted first"""
  E.check_encoder_regime(dev, name, other_entries=name in ('eval', 'ragged'))


def test_old_cases_never_left_the_one_row_regime():
  """What the three cases of test_feature_encoder reach on 256 CUs: one row per workgroup, no run crossing an image -- using the first image's
  coefficient table for a whole run, or never flushing the statistics at an image switch, changes nothing they compute."""
  for name in ('small', 'odd', 'wide'):
    c = E.cases.ENCODER_CASES[name]
    for s in E.encoder_splits(c['N'], c['H'], c['W'], 256):
      assert s['max_len'] == 1 and s['crossing'] == 0 and s['switching'] == 0


def test_encoder_rejects_images_below_16(dev):
  E.check_encoder_rejects_small_images(dev)


@pytest.mark.parametrize('name', ['dim', 'flat', 'const'])
def test_encoder_norm_statistics_conditioning(dev, name):
  """2 x 288 x 512 frames of 5 % / 1 % / no contrast: the kernels may be at most twice as far from float64 as the fp32 oracle is (floor: the
  encoder's 1e-4 + 1e-4 |ref|); forward-only kernels and the training form's forward"""
  E.check_encoder_conditioning(dev, name)


def test_encoder_norm_statistics_conditioning_six_term_build(dev):
  """the same three frames through libdynibar_hip_x6.so, in a subprocess because a process binds one library"""
  lib = os.path.join(ROOT, 'dynibar_amd', 'csrc', 'libdynibar_hip_x6.so')
  assert os.path.exists(lib), 'python -m dynibar_amd.build builds both engine variants'
  code = ("import sys; sys.path[:0] = [%r, %r]; import encoder_checks as E; from dynibar_amd import _lib; assert _lib.lib().dyn_mlp_split_terms() == 6\n"
          "for n in ('dim', 'flat', 'const'): E.check_encoder_conditioning('cuda:0', n)\n"
          "print('ok')") % (ROOT, os.path.join(ROOT, 'tests'))
  r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, DYNIBAR_HIP_LIB=lib), capture_output=True, text=True, timeout=900)
  print(r.stdout)
  assert r.returncode == 0 and 'ok' in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize('name', ['train', 'ragged'])
def test_encoder_training_form_at_the_training_shape(dev, name):
  """10 x 288 x 512 (weight-gradient GEMMs over 368,640 and 92,160 rows, 36 to 144 norm chunks per image) and 7 x 147 x 97: values and all 26
  parameter gradients against float64 autograd, and the run-to-run spread of two identical steps"""
  parity.check_encoder_training(dev, name, spread=True)


@pytest.mark.parametrize('k', [1, 3, 7])
def test_im2col(dev, k):
  for kk, stride, C, H, W in E.im2col_cases():
    if kk == k:
      E.check_im2col(dev, k, stride, C, H, W)


@pytest.mark.parametrize('k', [1, 3, 7])
def test_col2im_is_the_adjoint(dev, k):
  for kk, stride, C, H, W in E.im2col_cases(channels=(64,)):
    if kk == k:
      E.check_col2im(dev, k, stride, H, W)


@pytest.mark.parametrize('N', [1, 3])
def test_instance_norm_kernels(dev, N):
  for HW in E.IN_HW:
    for relu in (False, True):
      for with_res in (False, True):
        E.check_instance_norm(dev, HW, N, relu, with_res)


def test_instance_norm_kernels_far_from_zero_mean(dev):
  E.check_instance_norm_offset(dev)


def test_helper_argument_errors(dev):
  E.check_helper_argument_errors(dev)
