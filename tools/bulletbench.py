"""One bullet-time frame at the video shape (288 x 512, 7 + 3 temporal and virtual views, 15 static views, a 24-frame synthetic scene): the host
path of render_monocular_bt.py against the device-resident scene.  GPU only -- there is no CPU path.

  python tools/bulletbench.py [--seconds 1.0] [--rounds 5] [--frames 4] [--out profiles/bullet_time.txt]

Input assembly.  (a) the host path, what the package did before: the collated item of ``DynamicVideoDataset.__getitem__`` is on the host as
float32 (host_item() makes it once, outside the timed window: reading and DECODING the 26 images per frame, which the script does in its main
process, is NOT counted) and ``RaySamplerSingleImage(item, dev).get_all()`` copies it from pageable memory.  (b) ``scene.frame_sampler(plan)
.get_all()`` on a DeviceScene that was uploaded once (the upload and the view selection are not counted; the plan is fixed).
Output stage.  (a) the script's :342-361: ``.cpu()`` of rgb, rgb_static and rgb_dy, then clip, scale, cast and crop of rgb in numpy and the
stored frame beside it.  (b) ``scene.pack_frames([rgb], gt_frame=...)`` and one asynchronous copy of the packed bytes into pinned memory.
Each pair is checked to be bit-identical, then timed alternating in one process after warm-up, in rounds of at least --seconds each, with a
host clock around work that ends in a device synchronise.  The kernels' own times come from the library's per-kernel events in a separate
pass.  Last, --frames frames are rendered through dynibar_amd.bullet_time.frames (synthetic weights, 64 samples) and through the script's
loop body on the host path (items prepared beforehand), so that both stages can be set against a rendered frame of the same run.  No
speed-up is fixed in advance."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from scenebench import H, W, N_FRAMES, _stats, alternate, kernel_times, seeded_scene  # noqa: E402

RENDER_IDX, NUM_VV, NUM_SOURCE_VIEWS, MAX_RANGE, CROP = 11, 3, 7, 10, 0.03


def render_cameras(n, seed=5):
  import numpy as np
  from dynibar_amd import synthetic as syn
  rng = np.random.default_rng([seed, 17])
  K = np.eye(4)
  K[0, 0] = K[1, 1] = 0.8 * W
  K[0, 2], K[1, 2] = (W - 1) * 0.5, (H - 1) * 0.5
  return np.stack([syn.make_pose(rng, 0.4, 0.05) for _ in range(n)]), np.stack([K] * n)


def host_item(a, plan, K, gt_frame):
  """the collated item DynamicVideoDataset.__getitem__ returns for the plan's views (render_monocular_bt.py:157-259), on the host"""
  import numpy as np
  import torch
  idx = plan['render_idx']
  cam = lambda pose, intr: np.concatenate(([H, W], intr.flatten(), pose.flatten())).astype(np.float32)
  unit = lambda img: img.astype(np.float32) / 255.0
  src = [(unit(a['images'][i]), cam(a['poses'][i], a['intrinsics'][i])) for i in plan['nearest_pose_ids']]
  src += [(unit(a['virtual_views'][idx, v]), cam(a['virtual_poses'][idx, v], K)) for v in plan['virtual_ids']]
  static = [(unit(a['images'][i]) * (a['source_masks'][i].astype(np.float32) / 255.0)[..., None], cam(a['poses'][i], a['intrinsics'][i]))
            for i in plan['static_pose_ids']]
  T = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))[None]
  near, far = a['depth_range']
  return dict(camera=torch.from_numpy(plan['camera'])[None], rgb_path=[''], rgb=T(unit(a['images'][gt_frame])),
              src_rgbs=T(np.stack([r for r, _ in src])), src_cameras=T(np.stack([c for _, c in src])),
              static_src_rgbs=T(np.stack([r for r, _ in static])), static_src_cameras=T(np.stack([c for _, c in static])),
              depth_range=torch.tensor([[np.float64(near) * 0.9, np.float64(far) * 1.5]], dtype=torch.float64), ref_time=plan['data']['ref_time'],
              id=plan['data']['id'], nearest_pose_ids=plan['data']['nearest_pose_ids'])


def assert_same(got, want):
  import torch
  assert set(got) == set(want), sorted(set(got) ^ set(want))
  for k, w in want.items():
    if w is None:
      assert got[k] is None, k
    else:
      assert got[k].shape == w.shape and got[k].dtype == w.dtype and torch.equal(got[k], w), f'{k}: the device path and the host path differ'


def numpy_output_stage(images, gt_rgb):
  """render_monocular_bt.py:342-361 for device tensors rgb, rgb_static, rgb_dy and the item's rgb [1, H, W, 3]"""
  import numpy as np
  coarse_pred_rgb = images[0].detach().cpu()
  images[1].detach().cpu()
  images[2].detach().cpu()
  coarse_pred_rgb = (255 * np.clip(coarse_pred_rgb.numpy(), a_min=0, a_max=1.0)).astype(np.uint8)
  h, w = coarse_pred_rgb.shape[:2]
  crop_h, crop_w = int(h * CROP), int(w * CROP)
  coarse_pred_rgb = coarse_pred_rgb[crop_h:h - crop_h, crop_w:w - crop_w, ...]
  gt = gt_rgb[0, crop_h:h - crop_h, crop_w:w - crop_w, ...]
  gt = (255 * np.clip(gt.numpy(), a_min=0, a_max=1.)).astype(np.uint8)
  return np.concatenate([gt, coarse_pred_rgb], axis=1)


def make_model(dev):
  import torch
  from dynibar_amd import feature_network, synthetic as syn
  from frame_case import NUM_BASIS, dct_basis
  enc = lambda seed: feature_network.ResNet.from_module({k: torch.from_numpy(v).to(dev) for k, v in syn.make_encoder_weights(seed).items()})
  return types.SimpleNamespace(net_coarse_st=syn.make_weights('static', 0), net_coarse_dy=syn.make_weights('dynamic', 0),
                               motion_mlp=syn.make_weights('motion', 0, num_basis=NUM_BASIS), trajectory_basis=dct_basis(NUM_BASIS, N_FRAMES).to(dev),
                               feature_net=enc(0), feature_net_st=enc(1))


def run(seconds, rounds, n_frames):
  import numpy as np
  import torch
  from dynibar_amd import _lib, bullet_time, projection, render_image, sample_ray
  from dynibar_amd.scene import DeviceScene
  assert torch.cuda.is_available(), 'bulletbench needs an MI355X (there is no CPU path)'
  _lib.lib()
  dev = 'cuda:0'
  a = seeded_scene()
  scene = DeviceScene.for_rendering(dev, a['images'], a['intrinsics'], a['poses'], a['depth_range'], a['virtual_views'], a['virtual_poses'],
                                    a['source_masks'])
  args = types.SimpleNamespace(num_source_views=NUM_SOURCE_VIEWS, max_range=MAX_RANGE, num_vv=NUM_VV, mask_src_view=True, anti_alias_pooling=0,
                               mask_rgb=1, occ_weights_mode=0, chunk_size=8192, N_samples=64, inv_uniform=True, N_importance=0, white_bkgd=False)
  poses, intr = render_cameras(max(n_frames, 2))
  gt_frame = 0
  plan = scene.bullet_time_plan(poses[0], intr[0], RENDER_IDX, args, gt_frame=gt_frame)
  assert plan['counts'] == (7 + NUM_VV, 0, 2 * NUM_SOURCE_VIEWS + 1)
  data = host_item(a, plan, intr[0], gt_frame)

  # ---- input assembly
  host_in = lambda: sample_ray.RaySamplerSingleImage(data, dev).get_all()
  device_in = lambda: scene.frame_sampler(plan).get_all()
  assert_same(device_in(), host_in())
  t_hi, t_di = alternate((host_in, device_in), seconds, rounds)
  k_in = kernel_times(device_in)

  # ---- output stage
  g = torch.Generator(device=dev).manual_seed(7)
  images = [torch.rand((H, W, 3), generator=g, device=dev) * 1.4 - 0.2 for _ in range(3)]
  pinned = [None]

  def device_out():
    packed = scene.pack_frames(images[:1], CROP, gt_frame)
    if pinned[0] is None:
      pinned[0] = torch.empty(packed.shape, dtype=torch.uint8, pin_memory=True)
    pinned[0].copy_(packed, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return pinned[0].numpy()[0]

  host_out = lambda: numpy_output_stage(images, data['rgb'])
  assert np.array_equal(device_out(), host_out()), 'the packed frame differs from the numpy output stage'
  t_ho, t_do = alternate((host_out, device_out), seconds, rounds)
  k_out = kernel_times(device_out)

  # ---- rendered frames of the same run
  model, projector = make_model(dev), projection.Projector(dev)

  def device_frames():
    for f in bullet_time.frames(scene, model, projector, args, poses[:n_frames], intr[:n_frames], RENDER_IDX, with_gt=True):
      pass

  items = [data] + [host_item(a, scene.bullet_time_plan(poses[i], intr[i], RENDER_IDX, args, gt_frame=i), intr[i], i) for i in range(1, n_frames)]

  def host_frames_prepared():
    for i in range(n_frames):
      d = items[i]
      with torch.no_grad():
        smp = sample_ray.RaySamplerSingleImage(d, dev)
        rb = smp.get_all()
        cb, _ = model.feature_net(rb['src_rgbs'].squeeze(0).permute(0, 3, 1, 2))
        st, _ = model.feature_net_st(rb['static_src_rgbs'].squeeze(0).permute(0, 3, 1, 2))
        offs = [int(j - RENDER_IDX) for j in d['nearest_pose_ids'].squeeze().tolist()]
        ret = render_image.render_single_image_mono((RENDER_IDX, None), (d['ref_time'].to(dev), None), (offs, None), smp, rb, model, projector,
                                                    args.chunk_size, args.N_samples, args, inv_uniform=True, N_importance=0, det=True,
                                                    white_bkgd=False, featmaps=(cb, None, st), is_train=False, num_vv=NUM_VV)
      o = ret['outputs_coarse_ref']
      numpy_output_stage([o['rgb'], o['rgb_static'], o['rgb_dy']], d['rgb'])

  frame_ms = {}
  for name, f in (('host', host_frames_prepared), ('device', device_frames)):
    f()  # warm-up: packed weights, workspaces, pinned buffers
    torch.cuda.synchronize()
  for rnd in range(3):
    for name, f in (('host', host_frames_prepared), ('device', device_frames)):
      t0 = time.perf_counter()
      f()
      torch.cuda.synchronize()
      frame_ms.setdefault(name, []).append((time.perf_counter() - t0) / n_frames * 1e3)

  med = lambda ts: _stats([w for w, _ in ts])['median_ms']
  frame_dev, frame_host = _stats(frame_ms['device'])['median_ms'], _stats(frame_ms['host'])['median_ms']
  V = sum(plan['counts']) + 1
  hc, wc = H - 2 * int(H * CROP), W - 2 * int(W * CROP)
  host_bytes = sum(v.numel() * v.element_size() for v in data.values() if isinstance(v, torch.Tensor))
  return dict(metric='bullet_time_frame_stages_ms', shape=f'{H}x{W}', views=[7 + NUM_VV, 2 * NUM_SOURCE_VIEWS + 1], frames_resident=N_FRAMES,
              seconds_per_round=seconds, rounds=rounds, host_threads=torch.get_num_threads(), decoding_counted=False,
              input_host_path_wall=_stats([w for w, _ in t_hi]), input_device_path_wall=_stats([w for w, _ in t_di]),
              input_wall_ratio_host_over_device=round(med(t_hi) / med(t_di), 2),
              output_host_path_wall=_stats([w for w, _ in t_ho]), output_device_path_wall=_stats([w for w, _ in t_do]),
              output_wall_ratio_host_over_device=round(med(t_ho) / med(t_do), 2),
              host_item_megabytes=round(host_bytes / 1e6, 1), device_path_host_to_device_bytes=4 * (4 * V + 34),
              host_path_device_to_host_megabytes=round(3 * H * W * 3 * 4 / 1e6, 2), device_path_device_to_host_megabytes=round(hc * wc * 2 * 3 / 1e6, 2),
              pack_kernel_model_megabytes=dict(read=round((hc * wc * 12 + hc * wc * 3) / 1e6, 2), written=round(hc * wc * 6 / 1e6, 2)),
              kernel_ms={k: round(v, 5) for k, v in {**k_in, **k_out}.items()},
              rendered_frames=n_frames, rendered_frame_host_path=_stats(frame_ms['host']), rendered_frame_device_path=_stats(frame_ms['device']),
              input_share_of_frame=dict(host_path=round(med(t_hi) / frame_host, 4), device_path=round(med(t_di) / frame_dev, 4)),
              output_share_of_frame=dict(host_path=round(med(t_ho) / frame_host, 4), device_path=round(med(t_do) / frame_dev, 4)),
              bit_identical=True)


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--seconds', type=float, default=1.0)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--frames', type=int, default=4)
  ap.add_argument('--out', default=None, help='also write the result, one key per line, to this file')
  a = ap.parse_args()
  r = run(a.seconds, a.rounds, a.frames)
  print(json.dumps(r))
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(f'## python tools/bulletbench.py --seconds {a.seconds:g} --rounds {a.rounds} --frames {a.frames}   '
              f'(one bullet-time frame at {H} x {W}; times in ms per frame)\n')
      for k, v in r.items():
        f.write(f'{k}: {json.dumps(v)}\n')


if __name__ == '__main__':
  main()
