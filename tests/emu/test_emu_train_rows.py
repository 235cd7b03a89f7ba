"""The row kernels of csrc/dyn_train.hip one entry point at a time under the wave-level emulator: the same checks at the same shapes as
tests/test_gpu_train_rows.py (tests/train_rows.py).  Debugging aid in a container without a GPU; -m gpu is authoritative."""
import pytest

import train_rows

pytestmark = pytest.mark.emu


@pytest.mark.parametrize('name', sorted(train_rows.GROUPS))
def test_row_kernel(emu, name):
  train_rows.run_group(emu, name)


def test_act_bwd_above_a_million_rows(emu):
  train_rows.check_act_bwd_tall(emu)


def test_argument_errors(emu):
  train_rows.check_argument_errors(emu)
