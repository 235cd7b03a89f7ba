"""The logging branch of the reference's training loop (train.py:548-569 and log_view_to_tb, :576-762) on the gfx950 kernels.

    from utils import colorize                               ->   from dynibar_amd.view_log import colorize
    from ibrnet.data_loaders.flow_utils import flow_to_image ->   from dynibar_amd.view_log import flow_to_image
    log_view_to_tb(writer, global_step, args, ...)           ->   view_log.log_view(sampler, model, projector, args, ...).write(writer, global_step, 'train/')

Every ``i_img`` steps the script renders the current training frame with its anchor, builds twelve images from the result and hands them
to the summary writer.  ``panels`` builds the same twelve values -- the script's tags, shapes, dtypes and bits -- from the groups that
``render_single_image_mono`` leaves on the device with ``frame_outputs='device'``: three launches (csrc/dyn_viewlog.h: k_viewlog_ranges,
k_viewlog_flow_max, k_viewlog_panels) into one packed device buffer, and ``.cpu()`` brings that buffer to the host with one pinned copy.
Neither matplotlib nor cv2 is imported: the two colour maps the script uses are data (view_log_tables.py).

What is restated, and in whose arithmetic:
  * ``colorize(x, cmap_name)`` (utils.py:97-170) without mask or range: ``np.percentile(x, (1, 99))`` by the ``linear`` method with float64 results,
    ``vmax += 1e-6``, the clip, ``(x - vmin) / (vmax - vmin)`` and the clip to 0..1 in float64 (numpy >= 2 keeps a float64 scalar's precision
    against a float32 array; numpy < 2 would normalise in float32 and can land one table step away at a few pixels), then matplotlib's
    ``min(int(x * 256), 255)`` into the 256-entry table: float64 ``[H, W, 3]``.
  * ``flow_to_image(flow)`` (flow_utils.py:112-153 with compute_color and make_color_wheel): unknown pixels (``|u|`` or ``|v|`` above 200) count as
    0 and are painted black, ``maxrad`` in float32, everything from the divisor ``maxrad + eps`` on in float64: uint8 ``[H, W, 3]``.  The script's
    function zeroes the unknown pixels IN its argument; these functions never write to their inputs.
  * ``exp_sf_mag = torch.norm(exp_sf, dim=-1)`` on the host is ``sqrtf(fmaf(z, z, fmaf(y, y, x * x)))``, bit for bit.
Inputs must be finite.  ``mask``, ``range`` and ``append_cbar=True`` of ``colorize`` are not built and raise ``NotImplementedError``.  Tensors must be
on a HIP device: there is no CPU fallback, host tensors are refused.
"""
from __future__ import annotations

import ctypes
import types
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._lib import call, params, stream_of
from .train_static import POISON_SCRATCH
from .view_log_tables import TABLES

MAPS = tuple(TABLES)
MAX_IMAGES = 4   # scalar images per dyn_viewlog_ranges call, colour-mapped panels per dyn_viewlog_panels call
MAX_FLOWS = 12   # flow images per dyn_viewlog_flow_max / dyn_viewlog_panels call
MAX_RGB = 8
MAX_FLOW_STACK = 6  # train.py:732
RGB_TAGS = ('render_rgb_coarse_ref', 'render_rgb_coarse_anchor', 'render_rgb_static', 'render_rgb_dynamic', 'st_rgb_pred')
MAP_TAGS = ('render_depth_coarse', 'occ_weight_map', 'exp_sf_mag', 'gt_disp_coarse')
MAP_NAMES = ('jet', 'gray', 'gray', 'jet')  # train.py:704-717
TAGS = RGB_TAGS + MAP_TAGS + ('gt_rgb_coarse', 'rd_flow_stack', 'gt_flow_stack')
DATAFORMATS = {t: 'CHW' for t in TAGS[:10]}
DATAFORMATS.update(rd_flow_stack='NHWC', gt_flow_stack='NHWC')

_TABLE_CACHE = {}


def table(cmap_name, device=None):
  """The 256 x 3 float64 lookup table of a colour map: a host tensor, or the copy cached on ``device``."""
  if cmap_name not in TABLES:
    raise ValueError(f'unknown colour map {cmap_name!r}: this package ships {" and ".join(repr(m) for m in MAPS)}')
  key = (cmap_name, None if device is None else str(device))
  if key not in _TABLE_CACHE:
    host = torch.tensor([float.fromhex(v) for v in TABLES[cmap_name]], dtype=torch.float64).reshape(256, 3)
    _TABLE_CACHE[key] = host if device is None else host.to(device)
  return _TABLE_CACHE[key]


def percentile_plan(n):
  """What ``np.percentile(x, (1, 99))`` of n values derives from n alone (numpy/lib/_function_base_impl.py: percentile, _compute_virtual_index with
  alpha = beta = 1, _get_indexes, _get_gamma), in numpy's own float64 operations -> (rank int32 [4]: the indices of the order statistics
  below and above the 1st and the 99th percentile; weight float64 [2]: the interpolation weights)."""
  n = int(n)
  if n < 1:
    raise ValueError(f'a percentile of {n} values')
  q = np.true_divide(np.array([1, 99]), np.float32(100))  # the divisor takes the array's dtype; an int64 array over it is float64
  virtual = (n - 1) * q
  previous = np.floor(virtual)
  nxt = previous + 1
  above = virtual >= n - 1
  previous[above] = -1
  nxt[above] = -1
  previous, nxt = previous.astype(np.intp), nxt.astype(np.intp)
  weight = np.asarray(virtual - previous, dtype=np.float64)
  rank = np.stack([previous, nxt], axis=1).reshape(4)
  rank = np.where(rank < 0, rank + n, rank).astype(np.int32)
  return rank, weight


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def _check(t, what, dtype, shape_ok, shape_text):
  if not isinstance(t, torch.Tensor):
    raise ValueError(f'{what} must be a torch tensor on a HIP device, got {type(t).__name__}')
  if _lib._REQUIRE_DEVICE and not t.is_cuda:
    raise RuntimeError(f'dynibar_amd.view_log needs tensors on a HIP device (cuda:N), there is no CPU fallback; {what} is on {t.device}')
  if t.dtype != dtype:
    raise ValueError(f'{what} must be {str(dtype).replace("torch.", "")}, got {str(t.dtype).replace("torch.", "")}')
  if not shape_ok(tuple(t.shape)):
    raise ValueError(f'{what} must be {shape_text}, got {tuple(t.shape)}')
  if int(t.shape[0]) * int(t.shape[1]) * 3 >= 2 ** 31:
    raise ValueError(f'{what} is too large (H*W*3 < 2^31)')
  return t.detach().contiguous()


def _scalar_image(t, what):
  return _check(t, what, torch.float32, lambda s: len(s) == 2 and s[0] >= 1 and s[1] >= 1, '[H, W]')


def _vector_image(t, what, c):
  return _check(t, what, torch.float32, lambda s: len(s) == 3 and s[0] >= 1 and s[1] >= 1 and s[2] == c, f'[H, W, {c}]')


def _same(ts, what):
  if len({tuple(t.shape[:2]) for t in ts}) > 1 or len({t.device for t in ts}) > 1:
    raise ValueError(f'{what} must share one size and one device: ' + ', '.join(f'{tuple(t.shape)} on {t.device}' for t in ts))


def _scratch(shape, dtype, device):
  t = torch.empty(shape, dtype=dtype, device=device)
  if POISON_SCRATCH and dtype.is_floating_point:  # (train_static.py) under test the kernels must fill what is read later
    t.fill_(float('nan'))
  return t


def _plist(ts):
  """host list of device pointers -> (ctypes array kept alive by the caller, its address)"""
  arr = (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])
  return arr, ctypes.cast(arr, ctypes.c_void_p)


def _ilist(vs):
  arr = (ctypes.c_int32 * max(1, len(vs)))(*[int(v) for v in vs])
  return arr, ctypes.cast(arr, ctypes.c_void_p)


# ---- the three launches ------------------------------------------------------------------------------------------------------------
def ranges(images):
  """One ``dyn_viewlog_ranges`` launch: ``(vmin, vmax)`` of ``colorize`` for 1..4 images of one size.  An image is float32 ``[H, W]``, or float32
  ``[H, W, 3]`` whose magnitude is the image.  -> (float64 ``[K, 2]`` on the device, the K scalar images: the input itself or the magnitude)."""
  images = list(images)
  if not 1 <= len(images) <= MAX_IMAGES:
    raise ValueError(f'{len(images)} images in one call (1..{MAX_IMAGES})')
  ts = []
  for i, x in enumerate(images):
    is_mag = isinstance(x, torch.Tensor) and x.dim() == 3
    ts.append(_vector_image(x, f'image {i}', 3) if is_mag else _scalar_image(x, f'image {i}'))
  _same(ts, 'the images')
  H, W, dev = int(ts[0].shape[0]), int(ts[0].shape[1]), ts[0].device
  mags = [_scratch((H, W), torch.float32, dev) if t.dim() == 3 else None for t in ts]
  out = _scratch((len(ts), 2), torch.float64, dev)
  rank, weight = percentile_plan(H * W)
  img_keep, img_p = _plist(ts)
  mag_keep, mag_p = _plist([m if m is not None else ts[0] for m in mags])
  flag_keep, flag_p = _ilist([m is not None for m in mags])
  rank_keep, rank_p = _ilist(rank)
  w_keep = (ctypes.c_double * 2)(*[float(w) for w in weight])
  call('dyn_viewlog_ranges', len(ts), H, W, img_p, flag_p, mag_p, rank_p, ctypes.cast(w_keep, ctypes.c_void_p), ctypes.c_void_p(out.data_ptr()),
       stream_of(ts[0]))
  del img_keep, mag_keep, flag_keep, rank_keep
  return out, [m if m is not None else t for m, t in zip(mags, ts)]


def _flow_list(flows, what):
  flows = list(flows)
  if not 1 <= len(flows) <= MAX_FLOWS:
    raise ValueError(f'{len(flows)} flows in one call (1..{MAX_FLOWS})')
  ts = [_vector_image(f, f'{what} {i}', 2) for i, f in enumerate(flows)]
  _same(ts, 'the flows')
  return ts


def flow_max(flows):
  """One ``dyn_viewlog_flow_max`` launch: ``maxrad`` of ``flow_to_image`` for 1..12 flows, float32 ``[H, W, 2]`` of one size -> float32 ``[F]``."""
  ts = _flow_list(flows, 'flow')
  out = _scratch((len(ts),), torch.float32, ts[0].device)
  keep, p = _plist(ts)
  call('dyn_viewlog_flow_max', len(ts), int(ts[0].shape[0]), int(ts[0].shape[1]), p, ctypes.c_void_p(out.data_ptr()), stream_of(ts[0]))
  del keep
  return out


def _launch_panels(H, W, like, rgb=(), maps=(), flows=(), map_chw=True, flow_u8=False):
  """rgb: (src, clamp, dst); maps: (src, table, dst) with ``ranges`` rows in that order; flows: (src, dst) with ``maxrad`` entries in that order"""
  rgb, (map_list, rng), (flow_list, maxrad) = list(rgb), maps or ((), None), flows or ((), None)
  keep = [_plist([r[0] for r in rgb]), _ilist([r[1] for r in rgb]), _plist([r[2] for r in rgb]), _plist([m[0] for m in map_list]),
          _plist([m[1] for m in map_list]), _plist([m[2] for m in map_list]), _plist([f[0] for f in flow_list]), _plist([f[1] for f in flow_list])]
  p = params('DynViewLogPanelsParams', H=H, W=W, n_rgb=len(rgb), rgb_src=keep[0][1], rgb_clamp=keep[1][1], rgb_dst=keep[2][1],
             n_map=len(map_list), map_src=keep[3][1], map_table=keep[4][1], ranges=None if rng is None else ctypes.c_void_p(rng.data_ptr()),
             map_dst=keep[5][1], map_chw=1 if map_chw else 0, n_flow=len(flow_list), flow_src=keep[6][1],
             maxrad=None if maxrad is None else ctypes.c_void_p(maxrad.data_ptr()), flow_dst=keep[7][1], flow_u8=1 if flow_u8 else 0)
  call('dyn_viewlog_panels', p, stream_of(like))
  del keep


# ---- the two helpers of the script, device in, device out ----------------------------------------------------------------------------
def colorize(x, cmap_name='jet', mask=None, range=None, append_cbar=False, cbar_in_image=False):
  """``utils.colorize`` without mask, range and colour bar: float32 ``[H, W]`` on a HIP device -> float64 ``[H, W, 3]`` on that device (two launches)."""
  if mask is not None or range is not None or append_cbar:
    raise NotImplementedError('colorize: the mask, range and append_cbar=True options of the reference are not built')
  tab = table(cmap_name)  # (an unknown name is refused before anything else)
  x = _scalar_image(x, 'x')
  tab = table(cmap_name, x.device)
  H, W = int(x.shape[0]), int(x.shape[1])
  rng, (img,) = ranges([x])
  out = _scratch((H, W, 3), torch.float64, x.device)
  _launch_panels(H, W, x, maps=([(img, tab, out)], rng), map_chw=False)
  return out


def flow_to_image(flow, display=False):
  """``flow_utils.flow_to_image``: float32 ``[H, W, 2]`` on a HIP device -> uint8 ``[H, W, 3]`` on that device (two launches); ``flow`` is not changed."""
  if display:
    raise NotImplementedError('flow_to_image: display=True (a print of the flow range) is not built')
  (f,) = _flow_list([flow], 'flow')
  H, W = int(f.shape[0]), int(f.shape[1])
  maxrad = flow_max([f])
  out = torch.empty((H, W, 3), dtype=torch.uint8, device=f.device)
  _launch_panels(H, W, f, flows=([(f, out)], maxrad), flow_u8=True)
  return out


# ---- the twelve panels -------------------------------------------------------------------------------------------------------------
class Panels(OrderedDict):
  """tag -> tensor in the reference's order (TAGS), every entry a view into ONE packed buffer (``.buffer``, uint8)."""

  buffer = None

  def cpu(self):
    """The same mapping on the host: the packed buffer comes over in one copy (into pinned memory from a HIP device)."""
    buf = self.buffer
    if buf.is_cuda:
      host = torch.empty(buf.shape, dtype=buf.dtype, pin_memory=True)
      host.copy_(buf, non_blocking=True)
      torch.cuda.current_stream(buf.device).synchronize()
    else:
      host = buf.clone()
    out = Panels()
    out.buffer = host
    for tag, t in self.items():
      nbytes = t.numel() * t.element_size()
      off = t.data_ptr() - buf.data_ptr()
      out[tag] = host[off:off + nbytes].view(t.dtype).view(t.shape)
    return out

  def write(self, writer, global_step, prefix=''):
    """The twelve ``add_image`` / ``add_images`` calls of log_view_to_tb (train.py:680-759) in its order, on host tensors."""
    host = self.cpu() if self.buffer.is_cuda else self
    for tag in TAGS[:10]:
      writer.add_image(prefix + tag, host[tag], global_step, dataformats='CHW')
    for tag in TAGS[10:]:
      writer.add_images(prefix + tag, host[tag], global_step=global_step, dataformats='NHWC')
    return host


def panels(ret, gt_img, gt_disp, gt_flows):
  """log_view_to_tb's images (train.py:657-759) from a ``render_single_image_mono`` result whose groups are on the device
  (``frame_outputs='device'``), the frame's ``gt_img`` float32 ``[H, W, 3]``, ``gt_disp`` float32 ``[H, W, 1]`` or ``[H, W]`` and ``gt_flows`` float32
  ``[F, H, W, 2]`` or ``[F, H*W, 2]`` (``ray_batch['flows']``) on the same device.  -> Panels.  Three launches; no input is written."""
  ref, st, anchor = ret['outputs_coarse_ref'], ret['outputs_coarse_st'], ret['outputs_coarse_anchor']
  rgbs = [_vector_image(t, f'the rgb of {tag}', 3) for tag, t in
          zip(RGB_TAGS, (ref['rgb'], anchor['rgb'], ref['rgb_static'], ref['rgb_dy'], st['rgb']))]
  H, W = int(rgbs[0].shape[0]), int(rgbs[0].shape[1])
  if not isinstance(gt_img, torch.Tensor) or not isinstance(gt_disp, torch.Tensor) or not isinstance(gt_flows, torch.Tensor):
    raise ValueError('gt_img, gt_disp and gt_flows must be torch tensors on a HIP device')
  if gt_img.numel() != H * W * 3 or gt_disp.numel() != H * W or gt_flows.dim() < 3 or gt_flows[0].numel() != H * W * 2:
    raise ValueError(f'gt_img, gt_disp, gt_flows must hold a {H} x {W} frame, got {tuple(gt_img.shape)}, {tuple(gt_disp.shape)}, {tuple(gt_flows.shape)}')
  gt = _vector_image(gt_img.reshape(H, W, 3), 'gt_img', 3)
  n_flow = min(MAX_FLOW_STACK, int(gt_flows.shape[0]))  # train.py:732
  rd = ref['render_flows']
  if isinstance(rd, torch.Tensor) and rd.dim() == 3:  # (a single flow: the frame's reshape squeezes the leading axis away)
    rd = rd[None]
  if not isinstance(rd, torch.Tensor) or rd.dim() != 4 or rd.shape[0] < n_flow:
    raise ValueError(f'render_flows must hold {n_flow} flows [H, W, 2], got {tuple(getattr(rd, "shape", ()))}')
  gtf = gt_flows.reshape(gt_flows.shape[0], H, W, 2)
  flows = _flow_list([rd[i] for i in range(n_flow)] + [gtf[i] for i in range(n_flow)], 'flow')
  scal = [_scalar_image(ref['depth'], 'depth'), _scalar_image(anchor['occ_weight_map'], 'occ_weight_map'), _vector_image(ref['exp_sf'], 'exp_sf', 3),
          _scalar_image(gt_disp.reshape(H, W), 'gt_disp')]
  _same(rgbs + [gt] + flows + scal, 'the groups and the ground truth')
  dev, n = gt.device, H * W
  # the packed buffer: float64 panels first (8-byte aligned), then the float32 panels, then the two flow stacks
  sizes = [(tag, torch.float64, (3, H, W)) for tag in MAP_TAGS] + [(tag, torch.float32, (3, H, W)) for tag in RGB_TAGS + ('gt_rgb_coarse',)]
  sizes += [(tag, torch.float32, (n_flow, H, W, 3)) for tag in ('rd_flow_stack', 'gt_flow_stack')]
  total = sum(int(np.prod(s)) * (8 if d == torch.float64 else 4) for _, d, s in sizes)
  buf = torch.empty((total,), dtype=torch.uint8, device=dev)
  views, off = {}, 0
  for tag, d, s in sizes:
    nbytes = int(np.prod(s)) * (8 if d == torch.float64 else 4)
    views[tag] = buf[off:off + nbytes].view(d).view(s)
    off += nbytes
  rng, imgs = ranges(scal)
  maxrad = flow_max(flows)
  stacks = [views['rd_flow_stack'][i] for i in range(n_flow)] + [views['gt_flow_stack'][i] for i in range(n_flow)]
  _launch_panels(H, W, gt,
                 rgb=[(s, 1, views[tag]) for s, tag in zip(rgbs, RGB_TAGS)] + [(gt, 0, views['gt_rgb_coarse'])],
                 maps=([(img, table(name, dev), views[tag]) for img, name, tag in zip(imgs, MAP_NAMES, MAP_TAGS)], rng),
                 flows=(list(zip(flows, stacks)), maxrad))
  out = Panels()
  out.buffer = buf
  for tag in TAGS:
    out[tag] = views[tag]
  return out


def log_view(sampler, model, projector, args, num_dy_views, frame_idx, time_embedding, time_offset, render_stride=1):
  """train.py:548-569 with log_view_to_tb (:576-762) for a ``DeviceRaySampler`` (``scene.sampler(plan)``): switch_to_eval, the two encoder calls on
  the concatenated source views, the frame render with the groups left on the device, ``panels``, switch_to_train.  frame_idx, time_embedding
  and time_offset are the (ref, anchor) pairs of the training step.  -> Panels; writing them (``.write(writer, global_step, 'train/')``) is the
  caller's choice."""
  from . import render_image
  if render_stride != 1:
    raise NotImplementedError('log_view: render_stride != 1 (the training loop logs with render_stride=1)')
  H, W = sampler.H, sampler.W
  dev_args = types.SimpleNamespace(**vars(args))
  dev_args.frame_outputs = 'device'
  model.switch_to_eval()
  try:
    with torch.no_grad():
      ray_batch = sampler.get_all()
      gt_img = sampler.rgb.reshape(H, W, 3)
      gt_disp = sampler.disp.reshape(H, W, 1)
      if model.feature_net is not None:
        cb_src_rgbs = torch.cat([ray_batch['src_rgbs'].squeeze(0).permute(0, 3, 1, 2), ray_batch['anchor_src_rgbs'].squeeze(0).permute(0, 3, 1, 2)], dim=0)
        cb_featmaps_1, _ = model.feature_net(cb_src_rgbs)
        ref_featmaps, anchor_featmaps = cb_featmaps_1[0:num_dy_views], cb_featmaps_1[num_dy_views:]
        static_featmaps, _ = model.feature_net_st(ray_batch['static_src_rgbs'].squeeze(0).permute(0, 3, 1, 2))
        featmaps = (ref_featmaps, anchor_featmaps, static_featmaps)
      else:
        featmaps = [None, None]
      ret = render_image.render_single_image_mono(
          frame_idx=frame_idx, time_embedding=time_embedding, time_offset=time_offset, ray_sampler=sampler, ray_batch=ray_batch, model=model,
          projector=projector, chunk_size=args.chunk_size, N_samples=args.N_samples, args=dev_args, inv_uniform=args.inv_uniform, det=True,
          N_importance=args.N_importance, white_bkgd=args.white_bkgd, render_stride=render_stride, featmaps=featmaps, num_vv=args.num_vv)
      out = panels(ret, gt_img, gt_disp, ray_batch['flows'])
  finally:
    model.switch_to_train()
  return out
