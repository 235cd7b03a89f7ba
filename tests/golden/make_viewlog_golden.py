"""Golden vectors of the training loop's logged view panels, recorded from the REAL reference functions (build container only).

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_viewlog_golden.py

``utils.colorize`` and ``ibrnet/data_loaders/flow_utils.flow_to_image`` run as they are, with three shims: a stub ``cv2`` module whose ``resize`` returns
its input (and an ``INTER_AREA`` to name) (only the colour bar reaches it, and ``append_cbar=False`` throws the bar away), ``cm.get_cmap = lambda n: matplotlib.colormaps[n]``
(matplotlib 3.10 removed the old name), and flow_utils.py loaded by file path (so that data_loaders/__init__ does not pull in imageio).
Recorded for every data set and flow case of tests/view_log_cases.py at its GOLDEN_SHAPES: the input, ``colorize`` with both maps (float64
[H,W,3]) and ``flow_to_image`` (uint8 [H,W,3]; the function zeroes unknown pixels in its argument: it is handed a copy); vectors with their
``torch.norm(dim=-1)``; the numpy, matplotlib and torch versions.  -> tests/golden/view_log.npz (under 900 KB)
"""
import importlib.util
import os
import sys
import types

import matplotlib
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import refimport  # noqa: E402
import view_log_cases as vc  # noqa: E402

OUT = os.path.join(HERE, 'view_log.npz')
LIMIT = 900 * 1000
N_VECTORS = 6000


def reference_functions():
  sys.dont_write_bytecode = True
  if 'cv2' not in sys.modules:
    cv2 = types.ModuleType('cv2')
    cv2.resize = lambda img, *a, **k: img
    cv2.INTER_AREA = 3
    sys.modules['cv2'] = cv2
  from matplotlib import cm
  if not hasattr(cm, 'get_cmap'):
    cm.get_cmap = lambda n: matplotlib.colormaps[n]
  if refimport.REF_ROOT not in sys.path:
    sys.path.insert(0, refimport.REF_ROOT)
  import utils
  spec = importlib.util.spec_from_file_location('ref_flow_utils', os.path.join(refimport.REF_ROOT, 'ibrnet', 'data_loaders', 'flow_utils.py'))
  flow_utils = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(flow_utils)
  return utils.colorize, flow_utils.flow_to_image


def main():
  colorize, flow_to_image = reference_functions()
  out = {'versions': np.array([f'numpy {np.__version__}', f'matplotlib {matplotlib.__version__}', f'torch {torch.__version__}'])}
  for H, W in vc.GOLDEN_SHAPES:
    for name in vc.SCALAR_DATA:
      x = vc.scalar_data(name, H, W, fresh=True)
      out[f'colorize/{name}/{H}x{W}/x'] = x
      for cmap in vc.MAPS:
        y = colorize(torch.from_numpy(x.copy()), cmap_name=cmap, append_cbar=False)
        assert y.dtype == torch.float64 and tuple(y.shape) == (H, W, 3)
        out[f'colorize/{name}/{H}x{W}/{cmap}'] = y.numpy()
    for case in vc.FLOW_CASES:
      f = vc.flow_data(case, H, W, fresh=True)
      out[f'flow/{case}/{H}x{W}/flow'] = f
      img = flow_to_image(f.copy())
      assert img.dtype == np.uint8 and img.shape == (H, W, 3)
      out[f'flow/{case}/{H}x{W}/img'] = img
  v = vc.vector_data(N_VECTORS)
  out['norm/v'] = v
  out['norm/mag'] = torch.norm(torch.from_numpy(v), dim=-1).numpy()
  np.savez_compressed(OUT, **out)
  size = os.path.getsize(OUT)
  assert size < LIMIT, f'{OUT}: {size} bytes'
  print(OUT, size, 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
  main()
