"""dynibar_amd.criterion against the reference's own ibrnet/criterion.py + utils.img2charbonier: same values and same gradients, bit for bit,
for every helper train.py imports.  The reference's values and gradients on the seeded inputs of cases.criterion_cases are
tests/golden/criterion.npz (written by tests/golden/make_golden.py from the real reference)."""
import numpy as np
import pytest
import torch

import cases


@pytest.mark.parametrize('seed', list(cases.CRITERION_SEEDS))
def test_loss_helpers_match_the_reference(seed, golden_dir):
  import os
  import dynibar_amd.criterion as ours
  g = np.load(os.path.join(golden_dir, 'criterion.npz'))
  for name, fn, leaves in cases.criterion_cases(ours, seed):
    a, b = fn(), torch.from_numpy(g[f'seed{seed}/{name}/value'])
    assert torch.equal(a.detach(), b), f'{name}: {float(a)} vs {float(b)}'
    ga = torch.autograd.grad(a, leaves)
    assert len(ga) == sum(1 for k in g.files if k.startswith(f'seed{seed}/{name}/grad'))
    for i, x in enumerate(ga):
      assert torch.equal(x, torch.from_numpy(g[f'seed{seed}/{name}/grad{i}'])), f'{name}: gradients differ'
