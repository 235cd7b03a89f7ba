"""Golden items of the benchmark evaluation's dataset, recorded from the REAL reference class (build container only).

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_nvidia_item_golden.py

eval_nvidia.py cannot be imported where this runs (it imports cv2, imageio, skimage and `models` at the top; none is installed), so, as
make_golden_metrics.py does for a function, this takes the class ``DynamicVideoDataset`` out of the file with ``ast`` and executes it with
``np``, ``torch``, ``os`` and ``collections``; ``Dataset`` is ``object``, ``imageio.v2.imread`` serves the arrays of
eval_scene_cases.golden_scene from a dictionary of paths, ``cv2.resize`` is the identity for a nearest resize to the array's own size and
asserts exactly that.  ``__init__`` (which reads a dataset from disk) is bypassed with ``object.__new__`` and the attributes it sets are set
by hand; the real ``__getitem__`` then runs.

Recorded at 6 x 8 for N in 12, 14, 26, 30: every render_idx in 3 .. N - 4, cameras 0, 5 and 11 except the step's own, ``mask_static`` off and
on, bounds as float32 and as float64.  Every tensor of every item is compared with its neighbours here and stored once per value it can
depend on -- the image lists, their cameras, the masks and the ids per (N, mask_static, render_idx), which is where the static ids (not in
the item) go too; ``camera`` and ``rgb_path`` per (N, render_idx, camera); ``depth_range`` per (N, dtype of the bounds) -- and the generator
fails if an item differs along an axis it is not stored for.  -> tests/golden/nvidia_item.npz (data only)
"""
import ast
import collections
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import eval_scene_cases as ec  # noqa: E402
import refimport  # noqa: E402

STEP_KEYS = ('src_rgbs', 'src_cameras', 'static_src_rgbs', 'static_src_cameras', 'static_src_masks', 'nearest_pose_ids')


def reference_dataset_class(files):
  """DynamicVideoDataset with its readers stubbed.  files: {path: uint8 array}"""
  path = os.path.join(refimport.REF_ROOT, 'eval_nvidia.py')
  tree = ast.parse(open(path).read())
  cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'DynamicVideoDataset')

  def resize(x, dsize, interpolation=None):
    assert interpolation == 'nearest' and tuple(dsize) == (x.shape[1], x.shape[0]), 'the stub is the identity for a same-size nearest resize only'
    return x

  ns = {'np': np, 'torch': torch, 'os': os, 'collections': collections, 'Dataset': object,
        'imageio': types.SimpleNamespace(v2=types.SimpleNamespace(imread=lambda f: files[f])),
        'cv2': types.SimpleNamespace(resize=resize, INTER_NEAREST='nearest')}
  exec(compile(ast.Module(body=[cls], type_ignores=[]), path, 'exec'), ns)
  return ns['DynamicVideoDataset']


def dataset_of(cls, a, files, render_idx, mask_static, bounds):
  N = a['N']
  ds = object.__new__(cls)
  ds.folder_path, ds.render_idx, ds.mask_static = 'data', render_idx, mask_static
  ds.scene_path = ec.SCENE_PATH
  ds.num_frames = N
  ds.train_intrinsics, ds.train_poses = a['intrinsics'], a['poses']
  ds.train_rgb_files = [os.path.join(ec.SCENE_PATH, 'images_512x288', '%05d.png' % i) for i in range(N)]
  ds.render_intrinsics, ds.render_poses = a['intrinsics'], a['poses']
  ds.render_depth_range = [[bounds[0], bounds[1]]] * N
  ds.h, ds.w = [int(a['H'])] * N, [int(a['W'])] * N
  for i in range(N):
    files[ds.train_rgb_files[i]] = a['images'][i]
    files[os.path.join(ec.SCENE_PATH, 'coarse_masks', '%05d.png' % i)] = a['coarse_masks'][i]
  return ds


def same(x, y):
  if isinstance(x, torch.Tensor):
    return x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape) and torch.equal(x, y)
  if isinstance(x, np.ndarray):
    return x.dtype == y.dtype and np.array_equal(x, y)
  return type(x) is type(y) and x == y


def main():
  files = {}
  cls = reference_dataset_class(files)
  out = {'N': np.array(ec.GOLDEN_N), 'cams': np.array(ec.GOLDEN_CAMS), 'scene_path': np.array(ec.SCENE_PATH)}
  items = 0
  for N in ec.GOLDEN_N:
    a = ec.golden_scene(N)
    steps = list(range(3, N - 3))
    per = {(m, k): [] for m in (0, 1) for k in STEP_KEYS + ('static_ids', 'ref_time', 'id')}
    cameras, paths, depth = {}, {}, {}
    for render_idx in steps:
      for mask_static in (False, True):
        first = None
        for dtype in (np.float32, np.float64):
          ds = dataset_of(cls, a, files, render_idx, mask_static, ec.bounds_of(a, dtype))
          assert len(ds) == ec.NUM_CAMERAS
          for cam in ec.GOLDEN_CAMS:
            if cam == render_idx % ec.NUM_CAMERAS:
              continue
            item = ds[cam]
            items += 1
            assert set(item) == set(STEP_KEYS) | {'camera', 'rgb_path', 'depth_range', 'ref_time', 'id'}
            for k, v in item.items():  # the dtypes the tests rely on, as the reference returns them
              if isinstance(v, torch.Tensor) and k != 'depth_range':
                assert v.dtype == torch.float32, (k, v.dtype)
            assert item['depth_range'].dtype == (torch.float32 if dtype is np.float32 else torch.float64)
            if first is None:
              first = item
            for k in STEP_KEYS + ('ref_time', 'id'):
              assert same(item[k], first[k]), f'{k} depends on the camera or on the bounds (N={N}, render_idx={render_idx})'
            key = (render_idx, cam)
            for store, k in ((cameras, 'camera'), (paths, 'rgb_path')):
              assert key not in store or same(store[key], item[k]), f'{k} depends on mask_static or on the bounds'
              store[key] = item[k]
            dk = dtype.__name__
            assert dk not in depth or same(depth[dk], item['depth_range']), 'depth_range depends on more than the bounds'
            depth[dk] = item['depth_range']
        m = int(mask_static)
        for k in STEP_KEYS:
          per[(m, k)].append(np.asarray(first[k]))
        per[(m, 'ref_time')].append(first['ref_time'])
        per[(m, 'id')].append(first['id'])
        # the static ids are not in the item: read them off the cameras (every frame of the golden scene has a focal length of its own)
        focal = first['static_src_cameras'][:, 2].numpy().astype(np.float64)
        per[(m, 'static_ids')].append(np.round(focal - 8.0).astype(np.int64))
    out[f'N{N}/steps'] = np.array(steps)
    for (m, k), v in per.items():
      out[f'N{N}/mask{m}/{k}'] = np.stack(v) if k != 'ref_time' else np.array(v, dtype=np.float64)
    cases = ec.golden_cases(N)
    assert sorted(cameras) == sorted(cases)
    out[f'N{N}/cases'] = np.array(cases)
    out[f'N{N}/camera'] = np.stack([cameras[c].numpy() for c in cases])
    out[f'N{N}/rgb_path'] = np.array([paths[c] for c in cases])
    for dk, v in depth.items():
      out[f'N{N}/depth_range/{dk}'] = v.numpy()
    assert out[f'N{N}/depth_range/float32'].dtype == np.float32 and out[f'N{N}/depth_range/float64'].dtype == np.float64
    assert out[f'N{N}/mask1/src_rgbs'].dtype == np.float32 and out[f'N{N}/mask1/nearest_pose_ids'].dtype == np.int64
  path = os.path.join(HERE, 'nvidia_item.npz')
  np.savez_compressed(path, **out)
  print(f'wrote nvidia_item.npz: {items} items, {len(out)} arrays, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
  main()
