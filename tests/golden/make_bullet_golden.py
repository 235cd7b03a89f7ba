"""Golden vectors of the bullet-time view selection, recorded from the REAL reference functions (build container only).

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_bullet_golden.py

Only ibrnet/data_loaders/data_utils.py is loaded, by path, like make_scene_golden.py does.  Recorded, for each of scene_cases.GOLDEN_POSES
and bullet_cases.golden_render_poses of it (render poses that are not in the scene; for 'ties' one of them sits exactly on a lattice point,
so that equal distances occur): ``get_nearest_pose_ids(render_pose, poses, tar_id=-1, angular_dist_method='dist')`` and
``get_interval_pose_ids(render_pose, poses, tar_id=-1, angular_dist_method='dist', interval=k)`` for k in 1, 2, 3, 5.
-> tests/golden/bullet_plan.npz (a few KB, data only)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import bullet_cases as bc  # noqa: E402
import scene_cases as sc  # noqa: E402
from make_scene_golden import reference_data_utils  # noqa: E402


def main():
  du = reference_data_utils()
  out = {'names': np.array(sorted(sc.GOLDEN_POSES)), 'intervals': np.array(bc.GOLDEN_INTERVALS)}
  for name in sc.GOLDEN_POSES:
    poses, render = sc.golden_poses(name), bc.golden_render_poses(name)
    out[f'{name}/poses'], out[f'{name}/render_poses'] = poses, render
    out[f'{name}/nearest'] = np.stack([du.get_nearest_pose_ids(r, poses, tar_id=-1, angular_dist_method='dist') for r in render])
    for k in bc.GOLDEN_INTERVALS:
      out[f'{name}/interval{k}'] = np.stack([du.get_interval_pose_ids(r, poses, tar_id=-1, angular_dist_method='dist', interval=k) for r in render])
  np.savez_compressed(os.path.join(HERE, 'bullet_plan.npz'), **out)
  print('wrote bullet_plan.npz:', {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
  main()
