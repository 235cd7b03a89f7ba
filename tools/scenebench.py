"""One training batch at the training shape (288 x 512, 10 + 10 + 15 source views, 3072 rays): the host path against the device-resident scene.
GPU only -- there is no CPU path.

  python tools/scenebench.py [--seconds 1.0] [--rounds 5] [--out profiles/scene_batch.txt]

(a) the host path, what the package did before dynibar_amd.scene existed: the collated item of the data loader is on the host as float32
(host_item() makes it once, outside the timed window: decoding and stacking in the loader's workers are NOT counted), and
per batch ``RaySamplerSingleImage(data, dev).random_sample(3072, 'uniform')`` builds all rays, gathers on the host and copies about twenty
pageable tensors to the device.
(b) the device path: ``scene.sampler(plan).random_sample(3072, 'uniform')`` on a DeviceScene that was uploaded once (the upload is not counted,
nor is the view selection, which is the same host work in both paths; the plan is fixed so that both assemble the same 35 views).
Both are timed alternating in one process after warm-up, in rounds of at least --seconds each, with a host clock around work that ends in a
device synchronise (wall) and with HIP events on the stream around the same calls (device-side span of a batch, (b) only: (a)'s pageable
copies block the host, so its event span equals its wall time).  The view kernel's own time comes from the library's per-kernel events
(dyn_profile_*) in a separate pass, and is set against its byte model: V images of H*W*3 bytes read and 4 H*W*3 bytes written, plus the
masks of the static views, at the 6.29 TB/s a float4 copy reaches on this part (8.0 TB/s spec).  Both batches are checked to be bit-identical
before anything is timed.  No speed-up is fixed in advance."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, N_FRAMES, N_RAND = 288, 512, 24, 3072
HBM_COPY_TBS, HBM_SPEC_TBS = 6.29, 8.0


def _stats(xs):
  xs = sorted(xs)
  return dict(median_ms=round(xs[len(xs) // 2], 4), min_ms=round(xs[0], 4), max_ms=round(xs[-1], 4))


def seeded_scene(seed=3):
  """arrays as a loader holds them once per scene: random bytes for the images and masks, smooth camera motion, random supervision"""
  import numpy as np
  from dynibar_amd import synthetic as syn
  rng = np.random.default_rng([seed, H, W])
  N = N_FRAMES
  a = dict(images=rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8), virtual_views=rng.integers(0, 256, (N, 8, H, W, 3), dtype=np.uint8),
           source_masks=rng.integers(0, 256, (N, H, W), dtype=np.uint8))
  intr = np.tile(np.eye(4), (N, 1, 1))
  intr[:, 0, 0] = intr[:, 1, 1] = 0.78 * W
  intr[:, 0, 2], intr[:, 1, 2] = (W - 1) * 0.5, (H - 1) * 0.5
  a['intrinsics'] = intr
  a['poses'] = np.stack([syn.make_pose(rng, 0.4, 0.05) for _ in range(N)])
  a['virtual_poses'] = np.stack([[syn.make_pose(rng, 0.4, 0.05) for _ in range(8)] for _ in range(N)])
  a['depth_range'] = (1.0, 20.0)
  a['disp'] = (0.05 + 0.5 * rng.random((N, H, W))).astype(np.float32)
  a['motion_mask'] = (rng.random((N, H, W)) < 0.5).astype(np.uint8)
  a['static_mask'] = (rng.random((N, H, W)) < 0.3).astype(np.uint8)
  a['flows'] = rng.standard_normal((N, 6, H, W, 2), dtype=np.float32)
  a['flow_masks'] = (rng.random((N, 6, H, W)) < 0.8).astype(np.uint8)
  return a


def training_shape_plan(scene):
  """10 + 10 + 15 views: six neighbours and four virtual views at the target, seven neighbours and three virtual views at the anchor, fifteen
  masked static views"""
  idx, anchor = 11, 12
  plan = dict(idx=idx, anchor_idx=anchor, nearest_pose_ids=[idx + o for o in (1, 2, 3, -1, -2, -3)],
              anchor_nearest_pose_ids=sorted(anchor + o for o in (3, 2, 1, 0, -2, -3, -4)), static_pose_ids=[i for i in range(N_FRAMES) if i != idx][:15],
              ref_virtual=[0, 3, 5, 6], anchor_virtual=[1, 2, 7])
  plan['desc'], plan['counts'] = scene.descriptors(idx, anchor, plan['nearest_pose_ids'], plan['anchor_nearest_pose_ids'], plan['static_pose_ids'],
                                                   plan['ref_virtual'], plan['anchor_virtual'], True)
  assert plan['counts'] == (10, 10, 15)
  return plan


def host_item(a, plan):
  """the collated item MonocularDataset.__getitem__ returns for the plan's frames (monocular.py:120-144, :300-425), float32 on the host"""
  import numpy as np
  import torch

  def view(img, pose, intr, mask=None):
    rgb = img.astype(np.float32) / 255.0
    if mask is not None:
      rgb = rgb * (mask.astype(np.float32) / 255.0)[..., None]
    return rgb, np.concatenate((list(rgb.shape[:2]), intr.flatten(), pose.flatten())).astype(np.float32)

  idx, anc = plan['idx'], plan['anchor_idx']
  frame = lambda i, masked=False: view(a['images'][i], a['poses'][i], a['intrinsics'][i], a['source_masks'][i] if masked else None)
  virtual = lambda f, v: view(a['virtual_views'][f, v], a['virtual_poses'][f, v], a['intrinsics'][idx])
  lists = dict(src=[frame(i) for i in plan['nearest_pose_ids']] + [virtual(idx, v) for v in plan['ref_virtual']],
               anchor_src=[frame(i) for i in plan['anchor_nearest_pose_ids']] + [virtual(anc, v) for v in plan['anchor_virtual']],
               static_src=[frame(i, True) for i in plan['static_pose_ids']])
  T = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))[None]
  rgb, camera = frame(idx)
  data = dict(rgb=T(rgb), camera=T(camera), anchor_camera=T(frame(anc)[1]), disp=T(a['disp'][idx]), motion_mask=T(a['motion_mask'][idx]),
              static_mask=T(a['static_mask'][idx]), flows=T(a['flows'][idx]), masks=T(a['flow_masks'][idx]),
              depth_range=torch.tensor([[a['depth_range'][0] * 0.9, a['depth_range'][1] * 1.5]]).float(), rgb_path=['frame'])
  for k, vs in lists.items():
    data[k + '_rgbs'], data[k + '_cameras'] = T(np.stack([r for r, _ in vs])), T(np.stack([c for _, c in vs]))
  return data


def assert_same_batch(got, want):
  import numpy as np
  import torch
  assert set(got) == set(want), sorted(set(got) ^ set(want))
  for k, w in want.items():
    g = got[k]
    if w is None:
      assert g is None, k
    elif isinstance(w, np.ndarray):
      assert np.array_equal(g, w), k
    else:
      assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), f'{k}: the device path and the host path differ'


def alternate(fs, seconds, rounds, warmup=3):
  """time the callables alternating: per round each runs for at least `seconds`, synchronised at both ends -> per-call (wall ms, event ms) of every round"""
  import torch
  for _ in range(warmup):
    for f in fs:
      f()
  torch.cuda.synchronize()
  out = [[] for _ in fs]
  for _ in range(rounds):
    for f, dst in zip(fs, out):
      n, t0 = 0, time.perf_counter()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      while True:
        for _ in range(5):
          f()
        n += 5
        e1.record()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
          break
      dst.append((dt / n * 1e3, e0.elapsed_time(e1) / n))
  return out


def kernel_times(f, calls=50):
  """{kernel: mean ms} of the library's kernels over `calls` calls of f (HIP events around every launch)"""
  import torch
  from dynibar_amd import _lib
  lib = _lib.lib()
  nk = lib.dyn_profile_count()
  tot, cnt = (ctypes.c_float * nk)(), (ctypes.c_int * nk)()
  torch.cuda.synchronize()
  lib.dyn_profile_enable(1)
  lib.dyn_profile_read(tot, cnt)  # reset
  for _ in range(calls):
    f()
  torch.cuda.synchronize()
  lib.dyn_profile_read(tot, cnt)
  lib.dyn_profile_enable(0)
  return {lib.dyn_profile_name(i).decode(): tot[i] / cnt[i] for i in range(nk) if cnt[i]}


def run(seconds, rounds):
  import torch
  from dynibar_amd import _lib, sample_ray
  from dynibar_amd.scene import DeviceScene
  assert torch.cuda.is_available(), 'scenebench needs an MI355X (there is no CPU path)'
  _lib.lib()
  dev = 'cuda:0'
  a = seeded_scene()
  scene = DeviceScene(dev, a['images'], a['intrinsics'], a['poses'], a['depth_range'], a['disp'], a['motion_mask'], a['static_mask'], a['flows'],
                      a['flow_masks'], a['virtual_views'], a['virtual_poses'], a['source_masks'])
  plan = training_shape_plan(scene)
  data = host_item(a, plan)
  host = lambda: sample_ray.RaySamplerSingleImage(data, dev).random_sample(N_RAND, 'uniform')
  device = lambda: scene.sampler(plan).random_sample(N_RAND, 'uniform')
  sample_ray.rng.seed(1)
  want = host()
  sample_ray.rng.seed(1)
  assert_same_batch(device(), want)
  del want
  th, td = alternate((host, device), seconds, rounds)
  kt = kernel_times(device)
  V = sum(plan['counts'])
  image_bytes = H * W * 3
  model_bytes = V * image_bytes * 5 + plan['counts'][2] * H * W
  view_ms = kt['k_scene_views']
  host_bytes = sum(v.numel() * v.element_size() for v in data.values() if isinstance(v, torch.Tensor))
  return dict(metric='scene_batch_ms', shape=f'{H}x{W}', views=list(plan['counts']), rays=N_RAND, frames_resident=N_FRAMES,
              seconds_per_round=seconds, rounds=rounds, host_threads=torch.get_num_threads(),
              host_path_wall=_stats([w for w, _ in th]), device_path_wall=_stats([w for w, _ in td]), device_path_events=_stats([e for _, e in td]),
              wall_ratio_host_over_device=round(_stats([w for w, _ in th])['median_ms'] / _stats([w for w, _ in td])['median_ms'], 2),
              host_item_megabytes=round(host_bytes / 1e6, 1), device_path_host_to_device_bytes=4 * (4 * V + N_RAND),
              kernel_ms={k: round(v, 5) for k, v in kt.items()}, view_kernel_model_megabytes=round(model_bytes / 1e6, 2),
              view_kernel_tb_per_s=round(model_bytes / (view_ms * 1e-3) / 1e12, 3),
              view_kernel_fraction_of_copy_rate=round(model_bytes / (view_ms * 1e-3) / 1e12 / HBM_COPY_TBS, 3),
              view_kernel_fraction_of_spec=round(model_bytes / (view_ms * 1e-3) / 1e12 / HBM_SPEC_TBS, 3), bit_identical=True)


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--seconds', type=float, default=1.0)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--out', default=None, help='also write the result, one key per line, to this file')
  a = ap.parse_args()
  r = run(a.seconds, a.rounds)
  print(json.dumps(r))
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(f'## python tools/scenebench.py --seconds {a.seconds:g} --rounds {a.rounds}   (one training batch at {H} x {W}; times in ms per batch)\n')
      for k, v in r.items():
        f.write(f'{k}: {json.dumps(v)}\n')


if __name__ == '__main__':
  main()
