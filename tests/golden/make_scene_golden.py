"""Golden vectors of the static source-view ordering, recorded from the REAL reference function (build container only).

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_scene_golden.py

Only ibrnet/data_loaders/data_utils.py is loaded (by path: the package's __init__ chain imports cv2 and imageio, which are not installed); it
needs numpy and math.  Recorded: seeded camera-to-world poses -- scattered, with exact ties in the distance (mirrored and duplicated
positions), float32, and a longer scene -- and for every target frame the output of
``get_nearest_pose_ids(poses[t], poses, tar_id=t, angular_dist_method='dist')``.  -> tests/golden/scene_plan.npz (a few KB)
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import refimport  # noqa: E402
import scene_cases as sc  # noqa: E402


def reference_data_utils():
  sys.dont_write_bytecode = True
  path = os.path.join(refimport.REF_ROOT, 'ibrnet', 'data_loaders', 'data_utils.py')
  spec = importlib.util.spec_from_file_location('reference_data_utils', path)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def main():
  du = reference_data_utils()
  out = {'names': np.array(sorted(sc.GOLDEN_POSES))}
  for name in sc.GOLDEN_POSES:
    poses = sc.golden_poses(name)
    ids = np.stack([du.get_nearest_pose_ids(poses[t], poses, tar_id=t, angular_dist_method='dist') for t in range(len(poses))])
    out[f'{name}/poses'], out[f'{name}/ids'] = poses, ids
  np.savez_compressed(os.path.join(HERE, 'scene_plan.npz'), **out)
  print('wrote scene_plan.npz:', {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
  main()
