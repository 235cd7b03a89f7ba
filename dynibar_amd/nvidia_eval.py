"""The loop of the reference's ``eval_nvidia.py`` (:305-481) on a device-resident scene: the 12-camera benchmark evaluation,
``(N - 6) x 11`` target views per scene, without the script's per-view host work.

    scene = DeviceScene.for_evaluation(device, images_u8, intrinsics, c2w_mats, (near_depth, far_depth), coarse_masks=coarse_u8,
                                       gt_views=mv_images_u8, gt_masks=mv_masks_01)          # once per scene
    result = nvidia_eval.evaluate(scene, model, projector, args, on_step=lambda idx, moving: print(idx, moving))
    result['psnr'], result['ssim'], result['dynamic_psnr'], ...                             # the script's AVG numbers

Per TIME STEP: ``scene.eval_step_plan`` (the script's view selection, host integers), one launch that assembles both source-view lists, the
fp32 masks and the masked static views (``scene.assemble_eval_step``: one asynchronous host-to-device copy of a few hundred bytes) and the
four encoder passes of :335-358 -- the script repeats all of that for each of the step's 11 cameras although none of it depends on the
camera.  Per camera: 34 floats to the device, the rays, ``render_single_image_nvi`` with the script's arguments (its frame kept on the device:
``frame_outputs='device'``), the dynamic / static mask pair (``scene.eval_mask_pair``) and ``metrics.frame_sums`` into that camera's row of a
device table ``[11, 3, 3]``; with ``lpips=`` a ``dynibar_amd.lpips.LPIPS`` network, ``net.frame_sums`` on the same frame and masks into the same
row (the table is then ``[11, 9 + 30]``: both kernels' sums of a camera side by side).  After the step ONE asynchronous device-to-host copy brings the table into a pinned buffer; the numbers are
formed on the host with the reference's expressions once the event behind that copy has completed, while the next step is already queued.
Nothing is written to disk.  There is no CPU fallback: without the library or a HIP device every entry raises."""
from __future__ import annotations

import copy

import numpy as np
import torch

from . import metrics, render_image
from .lpips import lpips_of
from .view_selection import NUM_CAMERAS

SLOTS = 3  # pinned result buffers in rotation: a step's numbers are read before SLOTS - 1 further steps have been queued
NUMBERS = ('psnr', 'ssim', 'dynamic_psnr', 'dynamic_ssim', 'static_psnr', 'static_ssim')
LPIPS_NUMBERS = ('lpips', 'dynamic_lpips', 'static_lpips')  # added per view and to the means when a network is given


def encode_step(model, step):
  """The four encoder passes of eval_nvidia.py:335-358 on a step's tensors -> (coarse_featmaps, fine_featmaps) as the renderer takes them.
  Their inputs do not depend on the target camera: run once per time step."""
  src_rgbs = step.src_rgbs.squeeze(0).permute(0, 3, 1, 2)
  cb_featmaps_1, _ = model.feature_net(src_rgbs)
  static_src_rgbs = step.static_src_rgbs.squeeze(0).permute(0, 3, 1, 2)
  _, static_featmaps = model.feature_net(static_src_rgbs)
  cb_featmaps_1_fine, _ = model.feature_net_fine(src_rgbs)
  static_src_rgbs_ = step.static_src_rgbs_masked.squeeze(0).permute(0, 3, 1, 2)  # (without mask_static: static_src_rgbs itself)
  _, static_featmaps_fine = model.feature_net_fine(static_src_rgbs_)
  return (cb_featmaps_1, None, static_featmaps), (cb_featmaps_1_fine, None, static_featmaps_fine)


def render_view(scene, step, view_plan, featmaps, model, projector, args, render_args=None):
  """One target view: the sampler and ``render_single_image_nvi`` with the script's arguments (:360-378) -> (ret, ray_sampler)."""
  step_plan = view_plan['step']
  ref_frame_idx = int(step_plan['render_idx'])
  ref_time_offset = [int(near_idx - ref_frame_idx) for near_idx in step_plan['nearest_pose_ids'].tolist()]
  ray_sampler = scene.eval_sampler(step, view_plan)
  ray_batch = ray_sampler.get_all()
  ret = render_image.render_single_image_nvi(
      frame_idx=(ref_frame_idx, None), time_embedding=(step.ref_time, None), time_offset=(ref_time_offset, None), ray_sampler=ray_sampler,
      ray_batch=ray_batch, model=model, projector=projector, chunk_size=args.chunk_size, det=True, N_samples=args.N_samples,
      args=render_args if render_args is not None else args, inv_uniform=args.inv_uniform, N_importance=args.N_importance,
      white_bkgd=args.white_bkgd, coarse_featmaps=featmaps[0], fine_featmaps=featmaps[1], is_train=False)
  return ret, ray_sampler


def numbers_of(rows, H, W, taps=None):
  """the three rows of sums of one view (valid, dynamic, static) -> its numbers, with the reference's expressions (metrics._psnr_of / _ssim_of);
  ``taps``: the view's ``[3][5][2]`` table of dyn_lpips_frame, which adds the three LPIPS numbers"""
  out = {}
  for name, (sse, ssum, msum) in zip(('', 'dynamic_', 'static_'), rows):
    out[name + 'psnr'] = metrics._psnr_of(sse, msum)
    out[name + 'ssim'] = metrics._ssim_of(ssum, msum)
  out['valid_fraction'] = rows[0][2] / (3 * H * W)
  if taps is not None:
    for name, t in zip(('', 'dynamic_', 'static_'), taps):
      out[name + 'lpips'] = float(lpips_of(t))
  return out


def _queue_step(scene, model, projector, args, render_idx, data_range, lpips=None):
  """queues one time step on the device and its one copy back -> finish(): waits for that copy, -> the per-view dicts"""
  if not scene.has_ground_truth:
    raise ValueError('the evaluation needs a scene made by DeviceScene.for_evaluation with gt_views and gt_masks')
  render_idx = int(render_idx)
  step_plan = scene.eval_step_plan(render_idx, args)
  view_plans = [scene.eval_view_plan(step_plan, cam) for cam in range(NUM_CAMERAS) if cam != render_idx % NUM_CAMERAS]
  dev = scene.device
  render_args = copy.copy(args)
  render_args.frame_outputs = 'device'
  if hasattr(model, 'switch_to_eval'):
    model.switch_to_eval()
  with torch.no_grad():
    step = scene.assemble_eval_step(step_plan)
    featmaps = encode_step(model, step)
    V = len(view_plans)
    if lpips is None:
      table = metrics._scratch(V * 9, torch.float64, dev).view(V, 3, 3)
    else:  # both kernels' tables of a camera in one row: [3, 3] then [3, 5, 2]
      table = metrics._scratch(V * 39, torch.float64, dev).view(V, 39)
    for row, view_plan in enumerate(view_plans):
      ret, _ = render_view(scene, step, view_plan, featmaps, model, projector, args, render_args)
      fine_pred_rgb = ret['outputs_fine_ref']['rgb']
      masks = scene.eval_mask_pair(render_idx, view_plan['cam'])
      pred, gt = fine_pred_rgb.contiguous(), scene.gt_view(render_idx, view_plan['cam'])
      metrics.frame_sums(pred, gt, masks, data_range=data_range, apply_valid=True, valid_as_mask0=True,
                         out=table[row] if lpips is None else table[row, :9].view(3, 3))
      if lpips is not None:
        lpips.frame_sums(pred, gt, masks, apply_valid=True, valid_as_mask0=True, out=table[row, 9:].view(3, 5, 2))
  wait = scene.result_rotation(SLOTS).fetch(table)  # the time step's one device-to-host copy

  def finish():
    host = wait()
    if lpips is None:
      tables = [(r, None) for r in host.tolist()]
    else:
      tables = [(r[:9].view(3, 3).tolist(), r[9:].view(3, 5, 2).tolist()) for r in host]
    return [dict(render_idx=render_idx, cam=vp['cam'], rgb_path=vp['data']['rgb_path'][0], **numbers_of(r, scene.H, scene.W, t))
            for vp, (r, t) in zip(view_plans, tables)]

  return finish


def views(scene, model, projector, args, render_idx, data_range=metrics.REFERENCE_DATA_RANGE, lpips=None):
  """eval_nvidia.py:314-457 for the time step ``render_idx``, as a generator over its 11 target views (every camera but
  ``render_idx % 12``, in order).  The whole step is queued first; the views are yielded once its one device-to-host copy has completed.
  Yields dicts: ``render_idx``, ``cam``, ``rgb_path``, ``psnr``, ``ssim``, ``dynamic_psnr``, ``dynamic_ssim``, ``static_psnr``, ``static_ssim``,
  ``valid_fraction`` (Python floats), and with ``lpips=`` a ``dynibar_amd.lpips.LPIPS`` network ``lpips``, ``dynamic_lpips``, ``static_lpips``.  args: ``mask_static``, ``chunk_size``, ``N_samples``, ``N_importance``, ``inv_uniform``, ``white_bkgd`` and
  what the renderer reads.  ``data_range``: see dynibar_amd.metrics."""
  finish = _queue_step(scene, model, projector, args, render_idx, data_range, lpips)
  for view in finish():
    yield view


def evaluate(scene, model, projector, args, steps=None, on_step=None, data_range=metrics.REFERENCE_DATA_RANGE, lpips=None):
  """The script's loop over ``render_idx`` in ``3 .. N - 4`` (``steps``: another sequence of time steps).  Step i + 1 is queued before the
  numbers of step i are read.  ``on_step(render_idx, moving)`` receives the running means after every step: what the script prints as
  ``MOVING ...``.  -> dict: the six ``AVG`` numbers (``psnr``, ``ssim``, ``dynamic_psnr``, ``dynamic_ssim``, ``static_psnr``, ``static_ssim``:
  ``np.mean`` over all views so far, as the script forms them; with ``lpips=`` a network also ``lpips``, ``dynamic_lpips``, ``static_lpips``) and
  ``views``, the per-view table in the script's order."""
  steps = list(range(3, scene.N - 3)) if steps is None else [int(s) for s in steps]
  table = []

  def means():
    return {k: float(np.mean(np.array([v[k] for v in table]))) for k in (NUMBERS if lpips is None else NUMBERS + LPIPS_NUMBERS)}

  def take(finish, render_idx):
    table.extend(finish())
    if on_step is not None:
      on_step(render_idx, means())

  pending = None
  for render_idx in steps:
    finish = _queue_step(scene, model, projector, args, render_idx, data_range, lpips)
    if pending is not None:
      take(*pending)
    pending = (finish, render_idx)
  if pending is not None:
    take(*pending)
  if not table:
    raise ValueError('no time step to evaluate')
  out = means()
  out['views'] = table
  return out
