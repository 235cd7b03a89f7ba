"""-m gpu: the row kernels of csrc/dyn_train.hip one entry point at a time on the MI355X (tests/train_rows.py: equal on inputs whose sums are
exact, within twice an fp32 restatement's own error elsewhere)."""
import pytest
import torch

import train_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available(), 'the -m gpu tests need an MI355X'
  from dynibar_amd import _lib
  _lib.lib()  # fails loudly if the gfx950 library is missing
  return 'cuda:0'


@pytest.mark.parametrize('name', sorted(train_rows.GROUPS))
def test_row_kernel(dev, name):
  train_rows.run_group(dev, name)


def test_act_bwd_above_a_million_rows(dev):
  """rows >= 2^20 changes the rows per block of both forms of dyn_train_act_bwd: no other test has a matrix that tall"""
  train_rows.check_act_bwd_tall(dev)


def test_argument_errors(dev):
  train_rows.check_argument_errors(dev)
