"""One time step of the 12-camera benchmark evaluation at the evaluation shape (288 x 512, 7 temporal + 11 static views, a synthetic
24-frame scene with coarse masks, ground-truth views and dynamic masks): the host path of eval_nvidia.py against the device-resident scene.
GPU only -- there is no CPU path.

  python tools/evalscenebench.py [--seconds 0.5] [--rounds 3] [--steps 2] [--out profiles/nvidia_eval.txt]

(a) the host path, what the package did before: the collated item of ``DynamicVideoDataset.__getitem__`` is on the host as float32
(host_item() makes the step's 11 items once, outside the timed window: reading and DECODING the 18 images per view is NOT counted),
``RaySamplerSingleImage(item, dev).get_all()`` copies it from pageable memory, the four encoder passes run per view, the frame is rendered,
copied back (:380-381) and ``nvidia_frame_metrics`` uploads it again with the ground truth and the mask.  (b) ``dynibar_amd.nvidia_eval``:
one assembly launch and four encoder passes per time step, per view 34 floats, the rays, the render, the mask pair and the metrics into a
device table, one copy back per step.  Both paths alternate in one process after warm-up; the numbers of each pair of views are compared
bit for bit before anything is timed.  Timed: everything around the render per step and per view (host clock around work that ends in a
device synchronise), the whole loop body per view, the library's per-kernel event times of the two new kernels in a separate pass.  No ratio is
fixed in advance: the yardstick is the host path of the same process."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from scenebench import H, W, N_FRAMES, _stats, alternate, kernel_times  # noqa: E402

RENDER_IDX, CAMERAS = 11, 12


def seeded_scene(seed=4):
  import numpy as np
  from dynibar_amd import synthetic as syn
  rng = np.random.default_rng([seed, H, W])
  N = N_FRAMES
  a = dict(N=N, images=rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8), coarse_masks=rng.integers(0, 256, (N, H, W), dtype=np.uint8),
           gt_views=rng.integers(0, 256, (N, CAMERAS, H, W, 3), dtype=np.uint8), gt_masks=(rng.random((N, CAMERAS, H, W, 3)) < 0.3).astype(np.uint8))
  intr = np.tile(np.eye(4), (N, 1, 1))
  intr[:, 0, 0] = intr[:, 1, 1] = 0.78 * W
  intr[:, 0, 2], intr[:, 1, 2] = (W - 1) * 0.5, (H - 1) * 0.5
  a['intrinsics'] = intr
  a['poses'] = np.stack([syn.make_pose(rng, 0.4, 0.05) for _ in range(N)])
  a['bounds'] = (np.float32(1.0), np.float32(20.0 + 15.0))
  return a


def host_item(a, view_plan):
  """the collated item DynamicVideoDataset.__getitem__ returns for the view (eval_nvidia.py:121-198), on the host"""
  import numpy as np
  import torch
  plan, N = view_plan['step'], a['N']
  cam = lambda i: np.concatenate(([H, W], a['intrinsics'][i].flatten(), a['poses'][i].flatten())).astype(np.float32)
  unit = lambda img: img.astype(np.float32) / 255.0
  T = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))[None]
  ids, sids = plan['nearest_pose_ids'], plan['static_pose_ids']
  masks = [unit(a['coarse_masks'][i]) if (plan['mask_static'] and 3 <= i < N - 3) else np.ones((H, W), np.float32) for i in sids]
  near, far = a['bounds']
  return dict(camera=torch.from_numpy(view_plan['camera'])[None], rgb_path=view_plan['data']['rgb_path'],
              src_rgbs=T(np.stack([unit(a['images'][i]) for i in ids])), src_cameras=T(np.stack([cam(i) for i in ids])),
              static_src_rgbs=T(np.stack([unit(a['images'][i]) for i in sids])), static_src_cameras=T(np.stack([cam(i) for i in sids])),
              static_src_masks=T(np.stack(masks)), depth_range=torch.tensor([near * 0.9, far * 1.5])[None], ref_time=plan['data']['ref_time'],
              id=plan['data']['id'], nearest_pose_ids=plan['data']['nearest_pose_ids'])


def make_model(dev):
  import torch
  from dynibar_amd import feature_network, synthetic as syn
  from frame_case import NUM_BASIS, dct_basis
  enc = lambda seed: feature_network.ResNet.from_module({k: torch.from_numpy(v).to(dev) for k, v in syn.make_encoder_weights(seed).items()})
  basis = dct_basis(NUM_BASIS, N_FRAMES).to(dev)
  return types.SimpleNamespace(net_coarse_st=syn.make_weights('static', 0), net_coarse_dy=syn.make_weights('dynamic', 0),
                               net_fine_st=syn.make_weights('static', 100), net_fine_dy=syn.make_weights('dynamic', 100),
                               motion_mlp=syn.make_weights('motion', 0), motion_mlp_fine=syn.make_weights('motion', 100), trajectory_basis=basis,
                               trajectory_basis_fine=basis, feature_net=enc(0), feature_net_fine=enc(1))


def run(seconds, rounds, n_steps):
  import torch
  from dynibar_amd import _lib, metrics, nvidia_eval, projection, render_image, sample_ray
  from dynibar_amd.scene import DeviceScene
  assert torch.cuda.is_available(), 'evalscenebench needs an MI355X (there is no CPU path)'
  _lib.lib()
  dev = 'cuda:0'
  a = seeded_scene()
  scene = DeviceScene.for_evaluation(dev, a['images'], a['intrinsics'], a['poses'], a['bounds'], coarse_masks=a['coarse_masks'],
                                     gt_views=a['gt_views'], gt_masks=a['gt_masks'])
  args = types.SimpleNamespace(mask_static=True, anti_alias_pooling=1, mask_rgb=0, occ_weights_mode=0, chunk_size=8192, N_samples=64,
                               inv_uniform=True, N_importance=64, white_bkgd=False)
  model, projector = make_model(dev), projection.Projector(dev)
  plan = scene.eval_step_plan(RENDER_IDX, args)
  assert plan['counts'] == (7, 11)
  view_plans = [scene.eval_view_plan(plan, c) for c in range(CAMERAS) if c != RENDER_IDX % CAMERAS]
  items = [host_item(a, vp) for vp in view_plans]
  sync = lambda: torch.cuda.synchronize()

  # ---- the host path, stage by stage (eval_nvidia.py:332-358, :360-378, :380-457)
  def host_inputs(data):
    with torch.no_grad():
      smp = sample_ray.RaySamplerSingleImage(data, dev)
      rb = smp.get_all()
      src = rb['src_rgbs'].squeeze(0).permute(0, 3, 1, 2)
      st = rb['static_src_rgbs'].squeeze(0).permute(0, 3, 1, 2)
      ref_fm, _ = model.feature_net(src)
      _, st_fm = model.feature_net(st)
      ref_fm_f, _ = model.feature_net_fine(src)
      _, st_fm_f = model.feature_net_fine(st * rb['static_src_masks'].squeeze(0)[:, None, ...])
    return smp, rb, (ref_fm, None, st_fm), (ref_fm_f, None, st_fm_f)

  def host_render(data, smp, rb, cf, ff, render_args=args):
    offs = [int(j - RENDER_IDX) for j in data['nearest_pose_ids'].squeeze().tolist()]
    with torch.no_grad():
      return render_image.render_single_image_nvi((RENDER_IDX, None), (data['ref_time'].to(dev), None), (offs, None), smp, rb, model, projector,
                                                  args.chunk_size, args.N_samples, render_args, inv_uniform=True, N_importance=args.N_importance, det=True,
                                                  white_bkgd=False, coarse_featmaps=cf, fine_featmaps=ff, is_train=False)

  def host_numbers(rgb, depth, vp):
    rgb, depth = rgb.detach().cpu(), depth.detach().cpu()  # (:380-381; a frame the renderer already left on the host passes through)
    return metrics.nvidia_frame_metrics(rgb, a['gt_views'][RENDER_IDX, vp['cam']], a['gt_masks'][RENDER_IDX, vp['cam']].astype('float32'))

  def host_step():
    out = []
    for vp, data in zip(view_plans, items):
      ret = host_render(data, *host_inputs(data))
      out.append(host_numbers(ret['outputs_fine_ref']['rgb'], ret['outputs_fine_ref']['depth'], vp))
    return out

  device_step = lambda: list(nvidia_eval.views(scene, model, projector, args, RENDER_IDX))

  # ---- warm-up and the comparison, before anything is timed
  for f in (host_step, device_step):
    f()
    sync()
  want, got = host_step(), device_step()
  keys = nvidia_eval.NUMBERS + ('valid_fraction',)
  for vp, w, g in zip(view_plans, want, got):
    assert g['cam'] == vp['cam'] and {k: g[k] for k in keys} == w, f'camera {vp["cam"]}: the device path and the host path differ: {g} {w}'

  # ---- everything around the render
  on_device = types.SimpleNamespace(**{**vars(args), 'frame_outputs': 'device'})
  data0, vp0 = items[0], view_plans[0]
  ret = host_render(data0, *host_inputs(data0), render_args=on_device)
  rgb_dev, depth_dev = ret['outputs_fine_ref']['rgb'].contiguous(), ret['outputs_fine_ref']['depth'].contiguous()
  table = torch.empty((11, 3, 3), dtype=torch.float64, device=dev)
  pinned = torch.empty((11, 3, 3), dtype=torch.float64, pin_memory=True)
  state = {}

  def device_per_step():
    with torch.no_grad():
      state['step'] = scene.assemble_eval_step(plan)
      state['feat'] = nvidia_eval.encode_step(model, state['step'])
    pinned.copy_(table, non_blocking=True)

  def device_per_view():
    scene.eval_sampler(state['step'], vp0).get_all()
    metrics.frame_sums(rgb_dev, scene.gt_view(RENDER_IDX, vp0['cam']), scene.eval_mask_pair(RENDER_IDX, vp0['cam']),
                       data_range=metrics.REFERENCE_DATA_RANGE, apply_valid=True, valid_as_mask0=True, out=table[0])

  def host_per_view():
    host_inputs(data0)
    host_numbers(rgb_dev, depth_dev, vp0)

  device_per_step()
  t_hv, t_dv, t_ds = alternate((host_per_view, device_per_view, device_per_step), seconds, rounds)
  k_step = kernel_times(lambda: scene.assemble_eval_step(plan))
  k_pair = kernel_times(lambda: scene.eval_mask_pair(RENDER_IDX, vp0['cam']))

  # ---- the loop body per view
  body = {}
  for rnd in range(n_steps):
    for name, f in (('host', host_step), ('device', device_step)):
      sync()
      t0 = time.perf_counter()
      f()
      sync()
      body.setdefault(name, []).append((time.perf_counter() - t0) / len(view_plans) * 1e3)

  med = lambda ts: _stats([w for w, _ in ts])['median_ms']
  Vs, HW = plan['counts'][1], H * W
  host_bytes = sum(v.numel() * v.element_size() for v in data0.values() if isinstance(v, torch.Tensor))
  around_host, around_dev = med(t_hv), med(t_dv) + med(t_ds) / len(view_plans)
  return dict(metric='nvidia_eval_around_the_render_ms', shape=f'{H}x{W}', views=[7, Vs], frames_resident=N_FRAMES, views_per_step=len(view_plans),
              seconds_per_round=seconds, rounds=rounds, host_threads=torch.get_num_threads(), decoding_counted=False,
              host_path_per_view_wall=_stats([w for w, _ in t_hv]), device_path_per_view_wall=_stats([w for w, _ in t_dv]),
              device_path_per_step_wall=_stats([w for w, _ in t_ds]),
              around_the_render_per_view=dict(host_path=round(around_host, 4), device_path=round(around_dev, 4),
                                              ratio_host_over_device=round(around_host / around_dev, 2)),
              loop_body_per_view_host_path=_stats(body['host']), loop_body_per_view_device_path=_stats(body['device']), steps_timed=n_steps,
              kernel_ms={k: round(v, 5) for k, v in {**k_step, **k_pair}.items() if k in ('k_scene_views_masked', 'k_eval_mask_pair')},
              views_masked_kernel_model_megabytes=dict(read=round(((7 + Vs) * HW * 3 + Vs * HW) / 1e6, 2),
                                                       written=round(4 * ((7 + 2 * Vs) * HW * 3 + Vs * HW) / 1e6, 2)),
              host_path_bytes_per_view=dict(host_to_device=host_bytes + HW * 3 * 4 + HW * 3 + HW * 3 * 4, device_to_host=HW * 3 * 4 + HW * 4 + 72),
              device_path_bytes_per_view=dict(host_to_device=round(4 * 34 + 4 * (4 * (7 + Vs) + 2) / len(view_plans), 1),
                                              device_to_host=round(11 * 72 / len(view_plans), 1)),
              bit_identical=True)


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--seconds', type=float, default=0.5)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--steps', type=int, default=2)
  ap.add_argument('--out', default=None, help='also write the result, one key per line, to this file')
  a = ap.parse_args()
  r = run(a.seconds, a.rounds, a.steps)
  print(json.dumps(r))
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(f'## python tools/evalscenebench.py --seconds {a.seconds:g} --rounds {a.rounds} --steps {a.steps}   '
              f'(one time step of the benchmark evaluation at {H} x {W}, 11 views; times in ms)\n')
      for k, v in r.items():
        f.write(f'{k}: {json.dumps(v)}\n')


if __name__ == '__main__':
  main()
