"""Golden vectors of the evaluation's masked PSNR, recorded from the REAL reference function (build container only).

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py

eval_nvidia.py cannot be imported where this runs (it imports cv2, imageio, skimage and `models` at the top; none is installed), so this takes
the source of the one function ``calculate_psnr`` out of the file with ``ast`` and executes it with ``numpy`` and ``math`` only.  Recorded, at
24 x 40: the inputs (tests/metrics_restatement.make_case) and the function's outputs for every prediction and mask, the ``mse == 0 -> 0`` case
included.  ``calculate_ssim`` has no such golden: it calls skimage, which is not installed.  -> tests/golden/eval_metrics.npz
"""
import ast
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metrics_restatement as mr  # noqa: E402
import refimport  # noqa: E402

H, W = 24, 40


def reference_calculate_psnr():
  path = os.path.join(refimport.REF_ROOT, 'eval_nvidia.py')
  tree = ast.parse(open(path).read())
  fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'calculate_psnr')
  ns = {'np': np, 'math': math}
  exec(compile(ast.Module(body=[fn], type_ignores=[]), path, 'exec'), ns)
  return ns['calculate_psnr']


def main():
  psnr = reference_calculate_psnr()
  out = {'predictions': np.array(mr.PREDICTIONS), 'masks': np.array(mr.MASKS)}
  for name in mr.PREDICTIONS:
    c = mr.make_case(H, W, name)
    pred, gt, _ = mr.prepare(c['pred'], c['target'])
    out[f'{name}/gt'], out[f'{name}/pred'] = gt, pred
    for k in mr.MASKS:
      out[f'{name}/mask/{k}'] = c['masks'][k]
      out[f'{name}/psnr/{k}'] = np.float64(psnr(gt, pred, c['masks'][k]))  # (:400 calculate_psnr(gt_img, fine_pred_rgb, mask))
  assert out['identical/psnr/ones'] == 0 and out['noisy/psnr/zero'] == 0 and out['noisy/psnr/ones'] > 10
  np.savez_compressed(os.path.join(HERE, 'eval_metrics.npz'), **out)
  print('wrote eval_metrics.npz:', {k: float(v) for k, v in out.items() if '/psnr/' in k and k.startswith('noisy')})


if __name__ == '__main__':
  main()
