"""Training batches assembled on the device from a scene that is uploaded once.

The reference builds ``ray_batch`` in three host steps per iteration: ``MonocularDataset.__getitem__`` (ibrnet/data_loaders/monocular.py:146-425)
decodes about 30 images in a DataLoader worker and stacks them as float32, ``RaySamplerSingleImage`` builds all ``H*W`` rays, and
``random_sample`` (sample_ray.py:262-331) gathers the supervision with fancy indexing and copies about twenty tensors to the device.  Here the
scene lives on the device as uint8 / fp32 stores and an iteration's batch is two kernel launches (csrc/dyn_scene.h) driven by a few dozen
integers:

    scene = DeviceScene(device, images, intrinsics, poses, depth_range, disp, motion_mask, static_mask, flows, flow_masks,
                        virtual_views, virtual_poses, source_masks)              # once per scene
    plan = scene.plan(epoch, args)                 # replaces the DataLoader's __getitem__: the same draws from np.random in the same order
    train_data = plan['train_data']                # id, anchor_id, ref_time, anchor_time, nearest_pose_ids, ... as train.py reads them
    ray_sampler = scene.sampler(plan)              # replaces RaySamplerSingleImage(train_data, device)
    ray_batch = ray_sampler.random_sample(N_rand, sample_mode=..., center_ratio=...)

``random_sample`` and ``get_all`` return what ``dynibar_amd.sample_ray.RaySamplerSingleImage`` returns for the collated dictionary of the same
frame: the same keys, shapes, dtypes and bits.  The pixel indices come from ``sample_ray.rng`` by ``sample_random_pixel``'s own logic, so the
reference's index stream is unchanged and shared with the host sampler.

What stays host work of the caller, once per scene: reading and decoding the files.  ``cv2.resize``, the disk erosion of the motion mask
(monocular.py:177-204) and ``disp / scale`` have device forms in ``dynibar_amd.ingest`` (restated contracts, believed but not verified against
cv2 / skimage), and ``DeviceScene.from_decoded`` runs them in front of the constructor.  The constructors take the arrays as a loader produces
them, as host arrays or as torch tensors that are already on the scene's device; those are adopted without a round trip through the host (their 0 / 1 check brings back one boolean per store).

Bullet-time frames (render_monocular_bt.py) come from the same resident scene, which then needs no training stores:

    scene = DeviceScene.for_rendering(device, images, intrinsics, poses, depth_range, virtual_views, virtual_poses, source_masks)
    plan = scene.bullet_time_plan(render_pose, render_intrinsics, render_idx, args, gt_frame=i)   # DynamicVideoDataset.__getitem__'s selection
    ray_batch = scene.frame_sampler(plan).get_all()      # RaySamplerSingleImage(data, device).get_all(): keys, shapes, dtypes, bits
    packed = scene.pack_frames([rgb, rgb_static, rgb_dy], crop_ratio, gt_frame=i)                 # the script's output stage, uint8 on the device

(``dynibar_amd.bullet_time.frames`` is the loop around them.)

Host traffic per batch: the plan's descriptors and the pixel indices go through one pinned staging buffer -- one asynchronous host-to-device
copy, no device-to-host copy and no synchronisation.  There is no CPU fallback: without the library or a HIP device this module raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import warnings

import numpy as np
import torch

from . import _lib, sample_ray, view_selection
from ._lib import call, params, stream_of
from .train_static import POISON_SCRATCH
# (the constants, the two orderings and bullet_time_descriptors stay importable from here)
from .view_selection import (FLOW_OFFSETS, MAX_VIEWS, NUM_CAMERAS, NUM_VIRTUAL, _max_views, _np, _shape, bullet_time_descriptors,
                             interval_pose_ids_dist, nearest_pose_ids_dist)

_STAGE_SLOTS = 4     # pinned staging buffers in rotation: a slot is rewritten only after the copy that read it has completed


def _p(t):
  return None if t is None else ctypes.c_void_p(t.data_ptr())


def _host_tensor(x):
  """the array as a host tensor without a copy (a read-only array is only read: uploaded)"""
  with warnings.catch_warnings():
    warnings.simplefilter('ignore', UserWarning)
    return torch.from_numpy(np.ascontiguousarray(x))


def _adopt(x, what, device):
  """a torch tensor that already lives on the scene's device is taken as it is (checked with device operations, never brought to the host);
  anything else becomes a host array"""
  if isinstance(x, torch.Tensor) and x.device.type == device.type == 'cuda' and x.device.index == (
      device.index if device.index is not None else torch.cuda.current_device()):
    return x.detach().contiguous()
  return _np(x, what)


def _dtype(x):
  """'uint8', 'float32', ...: of a numpy array or of a torch tensor"""
  return str(x.dtype).replace('torch.', '')


def _binary_u8(x, want, what):
  """a 0 / 1 mask given as uint8, bool or float32 -> uint8 0 / 1 (a device tensor stays on its device)"""
  if isinstance(x, torch.Tensor) and x.is_cuda:
    _shape(x, want, what)
    if _dtype(x) not in ('uint8', 'bool', 'float32'):
      raise ValueError(f'{what} must be uint8, bool or float32, got {_dtype(x)}')
    if x.dtype != torch.bool and not bool(torch.logical_or(x == 0, x == 1).all()):
      raise ValueError(f'{what} must hold only 0 and 1')
    return x.to(torch.uint8).contiguous()
  x = _shape(_np(x, what), want, what)
  if x.dtype not in (np.uint8, np.bool_, np.float32):
    raise ValueError(f'{what} must be uint8, bool or float32, got {x.dtype}')
  if x.dtype != np.bool_ and not np.logical_or(x == 0, x == 1).all():
    raise ValueError(f'{what} must hold only 0 and 1')
  return np.ascontiguousarray(x.astype(np.uint8))


_TRAINING_STORES = ('disp', 'motion_mask', 'static_mask', 'flows', 'flow_masks')


def _need_training_stores(scene, what):
  missing = getattr(scene, 'missing_stores', ())
  if missing:
    made_by = getattr(scene, 'made_by', 'for_rendering')
    raise ValueError(f'{what} needs the training stores {", ".join(missing)}: this scene was made by DeviceScene.{made_by} without them')


def _need_virtual_views(scene, what):
  if getattr(scene, 'missing_views', False):
    raise ValueError(f'{what} needs the virtual views and their poses: this scene was made by DeviceScene.for_evaluation without them')


def _need_evaluation(scene, what):
  if getattr(scene, 'made_by', None) != 'for_evaluation':
    raise ValueError(f'{what} needs a scene made by DeviceScene.for_evaluation')


def _checked_lists(desc, counts, lists, least):
  """the descriptors as int32 ``[V, 4]`` and the sizes of their ``lists`` lists as ints -> (desc, V, counts); ValueError unless the sizes add up
  to ``V >= 1`` descriptors, every list has ``least`` views or more (None: not checked here) and none more than MAX_VIEWS"""
  desc = np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 4)
  V = int(desc.shape[0])
  counts = tuple(int(c) for c in counts)
  if len(counts) != lists or sum(counts) != V or V < 1 or (least is not None and min(counts) < least):
    raise ValueError(f'view lists of {counts} for {V} descriptors')
  _max_views(counts)
  return desc, V, counts


def _camera34(camera):
  camera = np.ascontiguousarray(camera, dtype=np.float32).reshape(-1)
  if camera.shape[0] != 34:
    raise ValueError(f'camera must hold 34 values [H, W, K, c2w], got {camera.shape[0]}')
  return camera


class ResultRotation(object):
  """``slots`` pinned host buffers with events in rotation, for results that come back from ``device`` while later work is already queued: a
  fetched buffer stays valid until ``slots - 1`` further results have been fetched."""

  def __init__(self, device, slots):
    self.device, self._slots, self._next = torch.device(device), [None] * slots, 0

  def fetch(self, t):
    """Queues the one asynchronous device-to-host copy of ``t`` into the next buffer (made anew where the shape or dtype changed) and records
    its event.  -> wait(): blocks until that copy has completed, -> the buffer, a host tensor that is reused later."""
    on_device = self.device.type == 'cuda'
    j, self._next = self._next, (self._next + 1) % len(self._slots)
    if self._slots[j] is None or self._slots[j][0].shape != t.shape or self._slots[j][0].dtype != t.dtype:
      self._slots[j] = (torch.empty(t.shape, dtype=t.dtype, pin_memory=on_device), torch.cuda.Event() if on_device else None)
    buf, ev = self._slots[j]
    with torch.cuda.device(self.device) if on_device else contextlib.nullcontext():
      buf.copy_(t, non_blocking=True)
      if ev is not None:
        ev.record()

    def wait():
      if ev is not None:
        ev.synchronize()
      return buf

    return wait


class DeviceScene(object):
  """One monocular scene of ``N >= 7`` frames, resident on ``device``.

  images         uint8 ``[N, H, W, 3]``: the decoded frames (the reference divides them by 255 per iteration; the kernels do it on the fly)
  intrinsics     ``[N, 4, 4]``, poses ``[N, 4, 4]`` camera-to-world (``batch_parse_llff_poses``); cast to float32 for the cameras like
                 ``load_src_view`` does, kept as given for the view selection
  depth_range    ``(near, far)``: becomes ``[near * 0.9, far * 1.5]``, computed in double and then cast to float32 (monocular.py:396-398)
  disp           float32 ``[N, H, W]``, already divided by the scene's scale
  motion_mask, static_mask   ``[N, H, W]``, flow_masks ``[N, 6, H, W]``: 0 / 1 as uint8, bool or float32 (after the caller's resize / erosion)
  flows          float32 ``[N, 6, H, W, 2]``; flows and flow_masks in the order of the offsets +1, +2, +3, -1, -2, -3
  virtual_views  uint8 ``[N, 8, H, W, 3]``, virtual_poses ``[N, 8, 4, 4]`` (``batch_parse_vv_poses``)
  source_masks   None, or the masks ``args.mask_src_view`` multiplies the static source views by (monocular.py:131-142): uint8 ``[N, H, W]``
                 or ``[N, H, W, 3]`` as decoded, 0..255 (the view is multiplied by ``m / 255``); bool or float32 0 / 1 are stored as 0 / 255

  Decoding is the caller's; ``cv2.resize``, the erosion and ``disp / scale`` are ``dynibar_amd.ingest``'s (``from_decoded``).  Every array may be a
  host array or a torch tensor on ``device`` (adopted in place: a float32 or uint8 store may alias it).  Bad shapes or dtypes raise ValueError."""

  def __init__(self, device, images, intrinsics, poses, depth_range, disp, motion_mask, static_mask, flows, flow_masks, virtual_views,
               virtual_poses, source_masks=None):
    self._setup(device, images, intrinsics, poses, depth_range, (disp, motion_mask, static_mask, flows, flow_masks), virtual_views, virtual_poses,
                source_masks)

  @classmethod
  def from_decoded(cls, device, frames, depth, dynamic_masks, static_masks, flows, flow_masks, virtual_views, virtual_poses, intrinsics, poses,
                   depth_range, scale, erosion_radius, size=None, source_masks=None, batch=None):
    """A training scene from what a caller has after DECODING a scene's files: ``dynibar_amd.ingest.prepare_monocular`` (the loader's resizes,
    the erosion of the motion mask and ``disp / scale`` on the device, ``batch`` frames at a time; its docstring has the arguments) followed by
    the constructor.  The full-resolution frames never pass through host-side resampling and no image data returns to the host; the
    constructor's 0 / 1 check of a mask that is already on the device reads back one boolean per store (a synchronisation, once per scene)."""
    from . import ingest
    prepared = ingest.prepare_monocular(frames, depth, dynamic_masks, static_masks, flows, flow_masks, virtual_views, virtual_poses, intrinsics,
                                        poses, depth_range, scale, erosion_radius, size=size, source_masks=source_masks,
                                        batch=batch or ingest.DEFAULT_BATCH, device=device)
    return cls(device, **prepared)

  @classmethod
  def for_rendering(cls, device, images, intrinsics, poses, depth_range, virtual_views, virtual_poses, source_masks=None):
    """A scene for ``bullet_time_plan`` / ``frame_sampler`` / ``pack_frames`` only: the arguments of the constructor without the training-only
    stores (disparity, motion and static masks, flows, flow masks).  ``plan``, ``sampler`` and ``assemble`` raise ValueError on it."""
    self = cls.__new__(cls)
    self._setup(device, images, intrinsics, poses, depth_range, None, virtual_views, virtual_poses, source_masks)
    return self

  @classmethod
  def for_evaluation(cls, device, images, intrinsics, poses, depth_range, coarse_masks=None, gt_views=None, gt_masks=None):
    """A scene of the 12-camera benchmark for ``eval_step_plan`` / ``eval_view_plan`` / ``eval_sampler`` / ``eval_mask_pair``
    (``dynibar_amd.nvidia_eval`` is the loop around them; eval_nvidia.py:24-198, :380-457).  It holds no virtual views and no training stores:
    ``plan``, ``sampler``, ``assemble``, ``bullet_time_plan`` and ``frame_sampler`` raise ValueError on it.

    images        uint8 ``[N, H, W, 3]``, ``N >= 12``; intrinsics, poses ``[N, 4, 4]`` (``batch_parse_llff_poses``)
    depth_range   ``(near, far)`` as the script has them after :46-48 (15 already added to ``far``).  The item's entry is
                  ``torch.tensor([near * 0.9, far * 1.5])`` on these very scalars (:184), so its dtype follows theirs: numpy float32 bounds
                  (``load_llff_data`` casts them) give float32, float64 bounds float64
    coarse_masks  None, or uint8 ``[N, H, W]``, 0..255 as decoded and resized: a static source view ``id`` with ``3 <= id < N - 3`` is later
                  multiplied by ``m / 255`` (``args.mask_static``, :156-169, :350-354).  One channel: the script's ``np.ones_like(src_rgb[..., 0])``
                  fixes ``[H, W]``, a three-channel array is refused
    gt_views      None, or uint8 ``[N, 12, H, W, 3]``: ``mv_images/%05d/cam%02d.jpg`` after the caller's ``cv2.resize(..., INTER_AREA)`` (:387-392)
    gt_masks      None, or 0 / 1 as uint8, bool or float32, ``[N, 12, H, W]`` or ``[N, 12, H, W, 3]``:
                  ``np.float32(cv2.imread(mv_masks...) > 1e-3)`` after the caller's nearest resize (:423-428)
    Entries of ``gt_views`` / ``gt_masks`` for frames outside ``3 .. N - 4`` are never read.

    Reading and decoding the files stays the caller's.  Both ``cv2.resize`` modes have device forms (``dynibar_amd.ingest.resize_area``,
    ``resize_nearest``): a caller can stream ``mv_images`` and the masks through them one time step at a time and pass device tensors here."""
    self = cls.__new__(cls)
    self._setup(device, images, intrinsics, poses, depth_range, None, None, None, coarse_masks, evaluation=(gt_views, gt_masks))
    return self

  def _setup(self, device, images, intrinsics, poses, depth_range, training, virtual_views, virtual_poses, source_masks, evaluation=None):
    """the constructor's checks and uploads; training: (disp, motion_mask, static_mask, flows, flow_masks), or None (for_rendering);
    evaluation: (gt_views, gt_masks) of for_evaluation, which has no virtual views, else None"""
    self.device = torch.device(device)
    self.made_by = 'for_evaluation' if evaluation is not None else 'for_rendering' if training is None else '__init__'
    self.missing_views = evaluation is not None
    self.missing_stores = () if training is not None else _TRAINING_STORES
    adopt = lambda x, what: _adopt(x, what, self.device)
    images = adopt(images, 'images')
    if _dtype(images) != 'uint8' or images.ndim != 4 or images.shape[3] != 3:
      raise ValueError(f'images must be uint8 [N, H, W, 3], got {_dtype(images)} {list(images.shape)}')
    N, H, W = (int(v) for v in images.shape[:3])
    if N < 7:
      raise ValueError(f'a scene needs at least 7 frames (the first and the last 3 are never targets), got {N}')
    if H < 1 or W < 1 or H * W * 3 >= 2 ** 31:
      raise ValueError(f'image size {H} x {W} is unsupported (H*W*3 < 2^31)')
    if evaluation is not None and N < NUM_CAMERAS:
      raise ValueError(f'an evaluation scene needs at least {NUM_CAMERAS} frames (one per camera of the benchmark), got {N}')
    self.N, self.H, self.W = N, H, W
    self.intrinsics_host = _shape(_np(intrinsics, 'intrinsics'), (N, 4, 4), 'intrinsics')
    self.poses_host = _shape(_np(poses, 'poses'), (N, 4, 4), 'poses')
    if training is not None:
      disp, motion_mask, static_mask, flows, flow_masks = training
      disp = _shape(adopt(disp, 'disp'), (N, H, W), 'disp')
      flows = _shape(adopt(flows, 'flows'), (N, 6, H, W, 2), 'flows')
      for x, what in ((disp, 'disp'), (flows, 'flows')):
        if _dtype(x) != 'float32':
          raise ValueError(f'{what} must be float32, got {_dtype(x)}')
      motion_mask = _binary_u8(adopt(motion_mask, 'motion_mask'), (N, H, W), 'motion_mask')
      static_mask = _binary_u8(adopt(static_mask, 'static_mask'), (N, H, W), 'static_mask')
      flow_masks = _binary_u8(adopt(flow_masks, 'flow_masks'), (N, 6, H, W), 'flow_masks')
    if evaluation is None:
      virtual_views = _shape(adopt(virtual_views, 'virtual_views'), (N, NUM_VIRTUAL, H, W, 3), 'virtual_views')
      if _dtype(virtual_views) != 'uint8':
        raise ValueError(f'virtual_views must be uint8, got {_dtype(virtual_views)}')
      virtual_poses = _shape(_np(virtual_poses, 'virtual_poses'), (N, NUM_VIRTUAL, 4, 4), 'virtual_poses')
    self.virtual_poses_host = virtual_poses  # as given: bullet_time_plan computes its distances in the caller's dtype
    mask_channels = 1
    gt_views = gt_masks = None
    if evaluation is not None:
      gt_views, gt_masks = evaluation
      if source_masks is not None:
        source_masks = adopt(source_masks, 'coarse_masks')
        if tuple(source_masks.shape) != (N, H, W):
          raise ValueError(f'coarse_masks must be [{N}, {H}, {W}] (one channel: the script builds its own all-ones mask as [H, W]), '
                           f'got {list(source_masks.shape)}')
        if _dtype(source_masks) != 'uint8':
          raise ValueError(f'coarse_masks must be uint8 (0..255 as decoded), got {_dtype(source_masks)}')
      if gt_views is not None:
        gt_views = _shape(adopt(gt_views, 'gt_views'), (N, NUM_CAMERAS, H, W, 3), 'gt_views')
        if _dtype(gt_views) != 'uint8':
          raise ValueError(f'gt_views must be uint8, got {_dtype(gt_views)}')
      if gt_masks is not None:
        gt_masks = adopt(gt_masks, 'gt_masks')
        if tuple(gt_masks.shape) not in ((N, NUM_CAMERAS, H, W), (N, NUM_CAMERAS, H, W, 3)):
          raise ValueError(f'gt_masks must be [{N}, {NUM_CAMERAS}, {H}, {W}] or [{N}, {NUM_CAMERAS}, {H}, {W}, 3], got {list(gt_masks.shape)}')
        gt_masks = _binary_u8(gt_masks, gt_masks.shape, 'gt_masks')
    if source_masks is not None:
      source_masks = adopt(source_masks, 'source_masks')
      if tuple(source_masks.shape) not in ((N, H, W), (N, H, W, 3)):
        raise ValueError(f'source_masks must be [{N}, {H}, {W}] or [{N}, {H}, {W}, 3], got {list(source_masks.shape)}')
      if _dtype(source_masks) != 'uint8':
        source_masks = _binary_u8(source_masks, source_masks.shape, 'source_masks')
        source_masks = source_masks * 255 if isinstance(source_masks, torch.Tensor) else source_masks * np.uint8(255)
      mask_channels = 3 if source_masks.ndim == 4 else 1
    if self.device.type != 'cuda' and _lib._REQUIRE_DEVICE:
      raise ValueError(f'DeviceScene needs a HIP device (cuda:N), got {self.device}: there is no CPU fallback')
    near, far = depth_range
    self.depth_range = torch.tensor([[near * 0.9, far * 1.5]]).float().to(self.device)  # [1, 2]: the collated form
    # (the bullet-time item has no .float(), render_monocular_bt.py:245: the script's numpy doubles stay float64 through default_collate)
    self.depth_range_f64 = torch.tensor([[float(near) * 0.9, float(far) * 1.5]], dtype=torch.float64).to(self.device)
    if evaluation is not None:  # (eval_nvidia.py:184 on the caller's scalars: the dtype is theirs; [1, 2] is the collated form)
      self.depth_range_eval = torch.tensor([near * 0.9, far * 1.5])[None].to(self.device)

    dev = self.device
    self._frames, image_stride = self._padded(images.reshape(N, -1))
    self._vviews = self._padded(virtual_views.reshape(N * NUM_VIRTUAL, -1))[0] if virtual_views is not None else None
    self._src_masks, mask_stride = self._padded(source_masks.reshape(N, -1)) if source_masks is not None else (None, 0)
    f32 = lambda x: x if isinstance(x, torch.Tensor) else _host_tensor(x.astype(np.float32, copy=False)).to(dev)  # (a device tensor: float32, adopted)
    u8 = lambda x: x if isinstance(x, torch.Tensor) else _host_tensor(x).to(dev)
    self._intrinsics = f32(self.intrinsics_host.reshape(N, 16))
    self._poses = f32(self.poses_host.reshape(N, 16))
    self._vposes = f32(virtual_poses.reshape(N, NUM_VIRTUAL, 16)) if virtual_poses is not None else None
    self._disp = self._flows = self._motion_mask = self._static_mask = self._flow_masks = None
    if training is not None:
      self._disp, self._flows = f32(disp), f32(flows)
      self._motion_mask, self._static_mask, self._flow_masks = u8(motion_mask), u8(static_mask), u8(flow_masks)
    self.has_source_masks = source_masks is not None
    self._image_stride = image_stride
    self._uv_grid = None
    self._store = params('DynSceneStore', N=N, H=H, W=W, image_stride=image_stride, frames=_p(self._frames), vviews=_p(self._vviews),
                         src_masks=_p(self._src_masks), mask_channels=mask_channels, mask_stride=mask_stride, intrinsics=_p(self._intrinsics),
                         poses=_p(self._poses), vposes=_p(self._vposes), disp=_p(self._disp), motion_mask=_p(self._motion_mask),
                         static_mask=_p(self._static_mask), flows=_p(self._flows), flow_masks=_p(self._flow_masks))
    self._stage_slots = [None] * _STAGE_SLOTS
    self._stage_next = self._stage_cap = 0  # (_upload)
    self._results = {}  # (result_rotation: slots -> ResultRotation)
    self.has_ground_truth = gt_views is not None and gt_masks is not None  # both stores of an evaluation scene: what nvidia_eval needs
    if evaluation is not None:
      self._gt_views = self._padded(gt_views.reshape(N * NUM_CAMERAS, -1))[0] if gt_views is not None else None
      self._gt_masks = self._padded(gt_masks.reshape(N * NUM_CAMERAS, -1))[0] if gt_masks is not None else None
      self.gt_mask_channels = 0 if gt_masks is None else 3 if gt_masks.ndim == 5 else 1

  def _padded(self, rows):
    """uint8 [n, bytes] -> the device store [n, stride], stride = bytes rounded up to 16 (zero padding), and the stride.  Rows already on the
    device that need no padding are adopted in place (the virtual views ``ingest.build_virtual_views`` made are not copied again)."""
    n, nbytes = rows.shape
    stride = (nbytes + 15) // 16 * 16
    if stride == nbytes and isinstance(rows, torch.Tensor) and rows.dtype == torch.uint8 and rows.is_contiguous():  # (a tensor: _adopt found it on the device)
      return rows, stride
    store = torch.zeros((n, stride), dtype=torch.uint8, device=self.device)
    store[:, :nbytes] = rows if isinstance(rows, torch.Tensor) else _host_tensor(rows).to(self.device)
    return store, stride

  def _out(self, *shape):
    t = torch.empty(shape, dtype=torch.float32, device=self.device)
    if POISON_SCRATCH:  # (train_static.py) under test: every element must be written by the kernels
      t.fill_(float('nan'))
    return t

  def _upload(self, *pieces):
    """The one host-to-device copy of a call: ``pieces`` (contiguous numpy arrays of int32, float32 or float64, taken as bit patterns) are written
    one after the other into the next slot of the pinned rotation and go to a fresh device int32 tensor in ONE asynchronous copy, whose event
    the slot keeps.  -> (the slot's host tensor, the device tensor): the pieces start at the same offsets in both.
    All slots grow together (a power of two, at least 1024 ints: after the first calls nothing is allocated); a slot whose last copy is still
    in flight is waited for (with _STAGE_SLOTS calls in between that copy finished long ago: no wait happens in a training loop)."""
    dev, on_device = self.device, self.device.type == 'cuda'
    pieces = [p.reshape(-1).view(np.int32) for p in pieces]
    n = sum([p.size for p in pieces])
    if n > self._stage_cap:
      self._stage_cap = max(1024, 1 << (n - 1).bit_length())
      for j, s in enumerate(self._stage_slots):
        if s is not None and s[2] is not None and s[3]:
          s[2].synchronize()
        host = torch.empty((self._stage_cap,), dtype=torch.int32, pin_memory=on_device)
        self._stage_slots[j] = [host, host.numpy(), torch.cuda.Event() if on_device else None, False]  # (buffer, its numpy view, event, used)
    slot = self._stage_slots[self._stage_next]
    self._stage_next = (self._stage_next + 1) % _STAGE_SLOTS
    host, stage, ev, used = slot
    if used and not ev.query():
      ev.synchronize()
    at = 0
    for p in pieces:
      stage[at:at + p.size] = p
      at += p.size
    ints = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev) if on_device else contextlib.nullcontext():
      ints.copy_(host[:n], non_blocking=True)
      if ev is not None:
        ev.record()
        slot[3] = True
    return host, ints

  def result_rotation(self, slots):
    """the scene's own ResultRotation of ``slots`` buffers, made at the first call for that count: the steps of an evaluation share it"""
    if slots not in self._results:
      self._results[slots] = ResultRotation(self.device, slots)
    return self._results[slots]

  # ---- training batches; the view selection is dynibar_amd/view_selection.py behind a check of the scene's stores -------------------------
  def plan(self, epoch, args, rng=np.random):
    """``view_selection.training_plan`` of this scene: ``MonocularDataset.__getitem__``'s selection, the same draws from ``rng`` in the same order"""
    _need_training_stores(self, 'plan')
    return view_selection.training_plan(self, epoch, args, rng)

  def descriptors(self, idx, anchor_idx, nearest_pose_ids, anchor_nearest_pose_ids, static_pose_ids, ref_virtual, anchor_virtual, mask_src_view):
    """``view_selection.training_descriptors`` of these lists (nothing of the scene is read)"""
    return view_selection.training_descriptors(idx, anchor_idx, nearest_pose_ids, anchor_nearest_pose_ids, static_pose_ids, ref_virtual,
                                               anchor_virtual, mask_src_view)

  def sampler(self, plan):
    _need_training_stores(self, 'sampler')
    return DeviceRaySampler(self, plan)

  def assemble(self, desc, counts, frame, anchor_frame, sel):
    """The two launches of one batch.  desc int32 ``[V, 4]``, counts the sizes of the three lists, sel the pixel indices (None: all ``H*W``).
    -> (images ``[V, H, W, 3]``, cameras ``[V, 34]``, dict of the per-pixel tensors and the two cameras).  Nothing synchronises."""
    _need_training_stores(self, 'assemble')
    H, W, out = self.H, self.W, self._out
    desc, V, counts = _checked_lists(desc, counts, 3, None)  # (an empty list is refused by ``descriptors`` and by the library)
    R = H * W if sel is None else int(len(sel))
    if R < 1:
      raise ValueError('no pixel selected')
    pieces = (desc,)
    if sel is not None:
      sel = np.asarray(sel)
      if sel.min() < -2 ** 31 or sel.max() >= 2 ** 31:
        raise ValueError('pixel index out of range')
      pieces = (desc, sel.astype(np.int32))
    host, ints = self._upload(*pieces)  # [desc | sel]: 4 (4 V + R) bytes
    images, cameras = out(V, H, W, 3), out(V, 34)
    st, hp, dp = stream_of(ints), host.data_ptr(), ints.data_ptr()
    call('dyn_scene_views', ctypes.byref(self._store), ctypes.c_void_p(hp), ctypes.c_void_p(dp), counts[0], counts[1], counts[2], _p(images),
         _p(cameras), st)
    px = dict(ray_o=out(R, 3), ray_d=out(R, 3), uv=out(R, 2), rgb=out(R, 3), disp=out(R), motion_mask=out(R), static_mask=out(R),
              flows=out(6, R, 2), masks=out(6, R, 1), camera=out(1, 34), anchor_camera=out(1, 34))
    p = params('DynSceneSupervisionParams', frame=int(frame), anchor_frame=int(anchor_frame), R=R,
               sel_host=None if sel is None else ctypes.c_void_p(hp + 16 * V), sel=None if sel is None else ctypes.c_void_p(dp + 16 * V),
               **{k: _p(v) for k, v in px.items()})
    call('dyn_scene_supervision', ctypes.byref(self._store), ctypes.byref(p), st)
    return images, cameras, px

  # ---- bullet-time frames (render_monocular_bt.py) --------------------------------------------------------------------------------
  def bullet_time_plan(self, render_pose, render_intrinsics, render_idx, args, gt_frame=None):
    """``view_selection.bullet_time_plan`` of this scene: the selection of render_monocular_bt.py's ``DynamicVideoDataset.__getitem__``"""
    _need_virtual_views(self, 'bullet_time_plan')
    return view_selection.bullet_time_plan(self, render_pose, render_intrinsics, render_idx, args, gt_frame)

  def frame_sampler(self, plan):
    _need_virtual_views(self, 'frame_sampler')
    return FrameRaySampler(self, plan)

  def uv_grid(self):
    """the pixel grid (x, y) of sample_ray.RaySamplerSingleImage, made once per scene by the same operations"""
    if self._uv_grid is None:
      ys, xs = torch.meshgrid(torch.arange(self.H, dtype=torch.float32, device=self.device),
                              torch.arange(self.W, dtype=torch.float32, device=self.device), indexing='ij')
      self._uv_grid = torch.stack([xs, ys], dim=-1).reshape(-1, 2)
    return self._uv_grid

  def assemble_frame(self, desc, counts, camera):
    """The two launches of one bullet-time frame.  desc int32 ``[V, 4]`` in three lists of ``counts`` views (the middle one: the ground-truth
    frame, or empty), camera float32 ``[34]``.  Descriptors and camera go to the device as bit patterns in ONE asynchronous copy from the
    pinned staging rotation; nothing comes back, nothing synchronises.
    -> (images ``[V, H, W, 3]``, cameras ``[V, 34]``, camera ``[1, 34]`` on the device, ray_o, ray_d ``[H*W, 3]``)"""
    H, W, out = self.H, self.W, self._out
    desc, V, counts = _checked_lists(desc, counts, 3, 0)
    host, ints = self._upload(desc, _camera34(camera))  # [desc | camera bits]: 4 (4 V + 34) bytes
    images, cameras, ray_o, ray_d = out(V, H, W, 3), out(V, 34), out(H * W, 3), out(H * W, 3)
    cam_dev = ints[4 * V:].view(torch.float32)
    st, hp, dp = stream_of(ints), host.data_ptr(), ints.data_ptr()
    call('dyn_scene_views_target', ctypes.byref(self._store), ctypes.c_void_p(hp), ctypes.c_void_p(dp), counts[0], counts[1], counts[2],
         ctypes.c_void_p(hp + 16 * V), ctypes.c_void_p(dp + 16 * V), _p(images), _p(cameras), st)
    call('dyn_image_rays', ctypes.c_void_p(dp + 16 * V), H, W, 1, _p(ray_o), _p(ray_d), st)  # the host sampler's own kernel: its bits
    return images, cameras, cam_dev[None], ray_o, ray_d

  def pack_frames(self, images, crop_ratio=0.03, gt_frame=None, out=None):
    """The output stage of render_monocular_bt.py:342-361 in one kernel.  images: 1..4 device fp32 tensors ``[H, W, 3]`` (``rgb``,
    ``rgb_static``, ``rgb_dy`` of ``outputs_coarse_ref``).  -> uint8 ``[K, H - 2 crop_h, (W - 2 crop_w) * (2 if gt_frame is not None else 1), 3]``
    on the device, ``crop = int(size * crop_ratio)``; every byte is ``(255 * np.clip(x, 0, 1)).astype(np.uint8)`` (NaN: 0), and with ``gt_frame``
    the cropped stored frame is the left half of every image.  ``out``: a tensor of that shape to write into."""
    images = list(images)
    K = len(images)
    if K < 1 or K > 4:
      raise ValueError(f'pack_frames takes 1..4 images, got {K}')
    for i, t in enumerate(images):
      if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f'image {i} must be a float32 tensor, got {getattr(t, "dtype", type(t).__name__)}')
      if t.dim() != 3 or t.shape[2] != 3 or tuple(t.shape) != tuple(images[0].shape):
        raise ValueError(f'image {i} must be [H, W, 3] like the first, got {list(t.shape)}')
      if t.device != images[0].device or (_lib._REQUIRE_DEVICE and not t.is_cuda):
        raise ValueError(f'image {i} is on {t.device}: the images must be on one HIP device')
    images = [t.detach().contiguous() for t in images]
    H, W = int(images[0].shape[0]), int(images[0].shape[1])
    if H * W * 3 >= 2 ** 31:
      raise ValueError(f'image size {H} x {W} is unsupported (H*W*3 < 2^31)')
    crop_h, crop_w = int(H * crop_ratio), int(W * crop_ratio)
    hc, wc = H - 2 * crop_h, W - 2 * crop_w
    if crop_h < 0 or crop_w < 0 or hc < 1 or wc < 1:
      raise ValueError(f'crop_ratio={crop_ratio} leaves no pixel of {H} x {W}')
    if gt_frame is not None:
      gt_frame = int(gt_frame)
      if (H, W) != (self.H, self.W):
        raise ValueError(f'the images are {H} x {W}, the stored frames {self.H} x {self.W}')
      if gt_frame < 0 or gt_frame >= self.N:
        raise ValueError(f'gt_frame={gt_frame} is outside the scene (0..{self.N - 1})')
    shape = (K, hc, wc * (2 if gt_frame is not None else 1), 3)
    if out is None:
      out = torch.empty(shape, dtype=torch.uint8, device=images[0].device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous()
          or out.device != images[0].device):
      raise ValueError(f'out must be a contiguous uint8 tensor {list(shape)} on {images[0].device}')
    p = params('DynFramePackParams', K=K, H=H, W=W, crop_h=crop_h, crop_w=crop_w, gt_frame=-1 if gt_frame is None else gt_frame, N=self.N,
               frames=_p(self._frames) if gt_frame is not None else None, image_stride=self._image_stride, out=_p(out),
               **{f'image{i}': _p(t) for i, t in enumerate(images)})
    call('dyn_frame_pack_u8', ctypes.byref(p), stream_of(out))
    return out

  # ---- the multi-camera benchmark evaluation (eval_nvidia.py) ---------------------------------------------------------------------------
  def eval_step_plan(self, render_idx, args):
    """``view_selection.eval_step_plan`` of this scene: the source views of one time step (they need no store: no check)"""
    return view_selection.eval_step_plan(self, render_idx, args)

  def eval_view_plan(self, step_plan, cam):
    """``view_selection.eval_view_plan`` of this scene: the target camera ``cam`` of a time step"""
    return view_selection.eval_view_plan(self, step_plan, cam)

  def assemble_eval_step(self, step_plan):
    """The one launch of a time step (dyn_scene_views_masked): both source-view lists, the fp32 masks and, with ``mask_static``, the masked
    static views the fine encoder is fed (eval_nvidia.py:350-354).  The descriptors go to the device in ONE asynchronous copy from the pinned
    staging rotation; nothing comes back, nothing synchronises.  -> EvalStep"""
    _need_evaluation(self, 'assemble_eval_step')
    H, W, out = self.H, self.W, self._out
    desc, V, (a, c) = _checked_lists(step_plan['desc'], step_plan['counts'], 2, 1)
    masked = bool(step_plan['mask_static'])
    ref_time = step_plan['data']['ref_time'].numpy().astype(np.float64).reshape(1)
    host, ints = self._upload(desc, ref_time)  # [desc | ref_time as a double]: 16 V + 8 bytes (16 V bytes in: the double is on 8 bytes)
    src, src_cams = out(a, H, W, 3), out(a, 34)
    st, st_cams, st_masks = out(c, H, W, 3), out(c, 34), out(c, H, W)  # (allocations of their own: every list starts on 16 bytes)
    st_masked = out(c, H, W, 3) if masked else None
    call('dyn_scene_views_masked', ctypes.byref(self._store), ctypes.c_void_p(host.data_ptr()), ctypes.c_void_p(ints.data_ptr()), a, c,
         1 if masked else 0, _p(src), _p(src_cams), _p(st), _p(st_cams), _p(st_masks), _p(st_masked), stream_of(ints))
    st = st[None]
    return EvalStep(step_plan, src[None], src_cams[None], st, st_cams[None], st_masks[None], st_masked[None] if masked else st,
                    ints[4 * V:].view(torch.float64))

  def eval_sampler(self, step, view_plan):
    """step: the EvalStep of ``view_plan['step']`` (``assemble_eval_step``), shared by the step's 11 cameras."""
    _need_evaluation(self, 'eval_sampler')
    return EvalRaySampler(self, step, view_plan)

  def eval_rays(self, camera):
    """The per-view part of an evaluation item: camera float32 ``[34]`` -> (camera ``[1, 34]`` on the device, ray_o, ray_d ``[H*W, 3]``).  One
    pinned asynchronous copy of the 34 floats and the host sampler's own kernel, dyn_image_rays, on the device copy: its bits."""
    H, W = self.H, self.W
    camera = _camera34(camera)
    if camera[0] != H or camera[1] != W:
      raise ValueError(f'the camera is {camera[0]:g} x {camera[1]:g}, the scene\'s images {H} x {W}')
    _, ints = self._upload(camera)  # [camera]: 136 bytes
    ray_o, ray_d = self._out(H * W, 3), self._out(H * W, 3)
    call('dyn_image_rays', ctypes.c_void_p(ints.data_ptr()), H, W, 1, _p(ray_o), _p(ray_d), stream_of(ints))
    return ints.view(torch.float32)[None], ray_o, ray_d

  def _gt_index(self, render_idx, cam, what):
    render_idx, cam = int(render_idx), int(cam)
    if render_idx < 0 or render_idx >= self.N:
      raise ValueError(f'{what}: render_idx={render_idx} is outside the scene (0..{self.N - 1})')
    if cam < 0 or cam >= NUM_CAMERAS:
      raise ValueError(f'{what}: cam={cam} is outside 0..{NUM_CAMERAS - 1}')
    return render_idx * NUM_CAMERAS + cam

  def gt_view(self, render_idx, cam):
    """the stored ground truth of camera ``cam`` at time ``render_idx``: a uint8 ``[H, W, 3]`` view of the store, no copy"""
    _need_evaluation(self, 'gt_view')
    if self._gt_views is None:
      raise ValueError('gt_view: the scene was made without gt_views')
    return self._gt_views[self._gt_index(render_idx, cam, 'gt_view'), :self.H * self.W * 3].view(self.H, self.W, 3)

  def eval_mask_pair(self, render_idx, cam, out=None):
    """The stored 0 / 1 dynamic mask of camera ``cam`` at time ``render_idx`` as the fp32 stack ``[2, H, W, C] = (m, 1.0f - m)`` that
    ``metrics.frame_sums`` takes as its user masks (eval_nvidia.py:423-444): one launch of dyn_eval_mask_pair, every element written.
    ``out``: a contiguous float32 tensor of that shape to write into."""
    _need_evaluation(self, 'eval_mask_pair')
    if self._gt_masks is None:
      raise ValueError('eval_mask_pair: the scene was made without gt_masks')
    H, W, C = self.H, self.W, self.gt_mask_channels
    row = self._gt_masks[self._gt_index(render_idx, cam, 'eval_mask_pair')]
    shape = (2, H, W, C)
    if out is None:
      out = self._out(*shape)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous()
          or out.device != row.device):
      raise ValueError(f'out must be a contiguous float32 tensor {list(shape)} on {row.device}')
    call('dyn_eval_mask_pair', _p(row), H, W, C, _p(out), stream_of(out))
    return out


class EvalStep(object):
  """The tensors of one time step of the evaluation, shared by its 11 target cameras: ``src_rgbs`` ``[1, 7, H, W, 3]``, ``src_cameras``
  ``[1, 7, 34]``, ``static_src_rgbs`` ``[1, Vs, H, W, 3]``, ``static_src_cameras`` ``[1, Vs, 34]``, ``static_src_masks`` ``[1, Vs, H, W]`` and
  ``static_src_rgbs_masked``: the product of eval_nvidia.py:350-354, or ``static_src_rgbs`` ITSELF without ``mask_static`` (the script's
  ``static_src_rgbs_ = static_src_rgbs``).  ``ref_time``: double ``[1]`` on the device, the script's ``data['ref_time'].cuda()``."""

  def __init__(self, plan, src_rgbs, src_cameras, static_src_rgbs, static_src_cameras, static_src_masks, static_src_rgbs_masked, ref_time):
    self.plan, self.ref_time = plan, ref_time
    self.src_rgbs, self.src_cameras = src_rgbs, src_cameras
    self.static_src_rgbs, self.static_src_cameras = static_src_rgbs, static_src_cameras
    self.static_src_masks, self.static_src_rgbs_masked = static_src_masks, static_src_rgbs_masked


_BATCH_KEYS = ('ray_o', 'ray_d', 'depth_range', 'camera', 'render_camera', 'anchor_camera', 'rgb', 'src_rgbs', 'src_cameras', 'anchor_src_rgbs',
               'anchor_src_cameras', 'static_src_rgbs', 'static_src_cameras', 'static_src_masks', 'disp', 'motion_mask', 'static_mask', 'uv_grid',
               'flows', 'masks')  # RaySamplerSingleImage.get_all's, in its order
_BATCH_OF_NONE = dict.fromkeys(_BATCH_KEYS)


def _ray_batch(**have):
  """the reference's key set, with None for every key a sampler does not have"""
  return {**_BATCH_OF_NONE, **have}


class DeviceRaySampler(object):
  """``RaySamplerSingleImage``'s contract (sample_ray.py) for one planned frame of a DeviceScene: ``.H``, ``.W``, ``.rgb``, ``.disp``, ``get_all()`` and
  ``random_sample(N_rand, sample_mode, center_ratio)``, with the values of the host sampler on the collated item of the same plan."""

  def __init__(self, scene, plan):
    self.scene, self.plan = scene, plan
    self.H, self.W = scene.H, scene.W
    self.device = scene.device
    self.render_stride = 1
    self.depth_range = scene.depth_range
    self._all = None

  def _batch(self, sel, **more):
    pl, c = self.plan, self.plan['counts']
    images, cameras, px = self.scene.assemble(pl['desc'], c, pl['idx'], pl['anchor_idx'], sel)
    a, b = c[0], c[0] + c[1]
    px['uv_grid'] = px.pop('uv')
    for k in ('disp', 'motion_mask', 'static_mask'):
      px[k] = px[k][:, None].squeeze()
    return _ray_batch(depth_range=self.depth_range, src_rgbs=images[None, :a], src_cameras=cameras[None, :a], anchor_src_rgbs=images[None, a:b],
                      anchor_src_cameras=cameras[None, a:b], static_src_rgbs=images[None, b:], static_src_cameras=cameras[None, b:], **px, **more)

  def get_all(self):
    """All rays of the frame with the per-view tensors (``RaySamplerSingleImage.get_all``)."""
    if self._all is None:
      self._all = self._batch(None)
    return dict(self._all)

  @property
  def rgb(self):
    return self.get_all()['rgb']  # [H*W, 3]

  @property
  def disp(self):
    return self.get_all()['disp'].reshape(-1, 1)  # [H*W, 1]

  def sample_random_pixel(self, N_rand, sample_mode, center_ratio=0.8):
    """``RaySamplerSingleImage.sample_random_pixel``: the same draws from ``sample_ray.rng``."""
    if sample_mode == 'center':
      border_H = int(self.H * (1 - center_ratio) / 2.0)
      border_W = int(self.W * (1 - center_ratio) / 2.0)
      u, v = np.meshgrid(np.arange(border_H, self.H - border_H), np.arange(border_W, self.W - border_W))
      u = u.reshape(-1)
      v = v.reshape(-1)
      if N_rand > u.shape[0]:
        raise ValueError(f'N_rand={N_rand} is larger than the pool of {u.shape[0]} centre pixels')
      select_inds = sample_ray.rng.choice(u.shape[0], size=(N_rand,), replace=False)
      select_inds = v[select_inds] + self.W * u[select_inds]
    elif sample_mode == 'uniform':
      if N_rand > self.H * self.W:
        raise ValueError(f'N_rand={N_rand} is larger than the pool of {self.H * self.W} pixels')
      select_inds = sample_ray.rng.choice(self.H * self.W, size=(N_rand,), replace=False)
    else:
      raise NotImplementedError
    return select_inds

  def random_sample(self, N_rand, sample_mode, center_ratio=0.8):
    """Random pixel batch with its supervision (``RaySamplerSingleImage.random_sample``), assembled on the device."""
    if N_rand < 1:
      raise ValueError(f'N_rand={N_rand}')
    select_inds = self.sample_random_pixel(N_rand, sample_mode, center_ratio)
    batch = self._batch(select_inds, selected_inds=select_inds)
    del batch['render_camera']  # (sample_ray.py:262-331 has no such key)
    return batch


class FrameRaySampler(object):
  """``RaySamplerSingleImage``'s contract for one bullet-time frame of a DeviceScene (``bullet_time_plan``): ``.H``, ``.W``, ``.render_stride``,
  ``.rgb`` and ``get_all()``, with the values of the host sampler on the collated item of ``DynamicVideoDataset.__getitem__``
  (render_monocular_bt.py:96-259).  ``rgb`` is the stored frame ``gt_frame`` / 255, or None without one."""

  def __init__(self, scene, plan):
    self.scene, self.plan = scene, plan
    self.H, self.W = scene.H, scene.W
    self.device = scene.device
    self.render_stride = 1
    self.depth_range = scene.depth_range_f64
    self._all = None

  def get_all(self):
    if self._all is None:
      pl, sc = self.plan, self.scene
      a, _, c = pl['counts']
      desc, g = pl['desc'], 0
      if pl['gt_frame'] is not None:  # the frame's own image is one more view of the same launch
        g = 1
        desc = np.concatenate([desc[:a], np.array([[pl['gt_frame'], -1, -1, pl['gt_frame']]], dtype=np.int32), desc[a:]], axis=0)
      images, cameras, camera, ray_o, ray_d = sc.assemble_frame(desc, (a, g, c), pl['camera'])
      self._all = _ray_batch(ray_o=ray_o, ray_d=ray_d, depth_range=self.depth_range, camera=camera, rgb=images[a].reshape(-1, 3) if g else None,
                             src_rgbs=images[None, :a], src_cameras=cameras[None, :a], static_src_rgbs=images[None, a + g:],
                             static_src_cameras=cameras[None, a + g:], uv_grid=sc.uv_grid())
    return dict(self._all)

  @property
  def rgb(self):
    return self.get_all()['rgb']  # [H*W, 3] or None

  def random_sample(self, N_rand, sample_mode, center_ratio=0.8):
    raise NotImplementedError('a bullet-time frame is rendered whole: get_all()')


class EvalRaySampler(object):
  """``RaySamplerSingleImage``'s contract for one target view of the benchmark evaluation (``eval_view_plan``): ``.H``, ``.W``,
  ``.render_stride``, ``.rgb_path`` and ``get_all()``, with the values of the host sampler on the collated item of
  ``DynamicVideoDataset.__getitem__`` (eval_nvidia.py:71-198).  The item has no ``rgb``: that key is None like every other key it lacks.
  ``static_src_rgbs_masked`` (the step's, :350-354) is an attribute, not a key: the key set stays the reference's."""

  def __init__(self, scene, step, view_plan):
    if step.plan is not view_plan['step']:
      raise ValueError('the view plan belongs to another time step than the assembled step')
    self.scene, self.step, self.plan = scene, step, view_plan
    self.H, self.W = scene.H, scene.W
    self.device = scene.device
    self.render_stride = 1
    self.depth_range = scene.depth_range_eval
    self.rgb_path = view_plan['data']['rgb_path']
    self.static_src_rgbs_masked = step.static_src_rgbs_masked
    self.rgb = None
    self._all = None

  def get_all(self):
    if self._all is None:
      sc, st = self.scene, self.step
      camera, ray_o, ray_d = sc.eval_rays(self.plan['camera'])
      self._all = _ray_batch(ray_o=ray_o, ray_d=ray_d, depth_range=self.depth_range, camera=camera, src_rgbs=st.src_rgbs,
                             src_cameras=st.src_cameras, static_src_rgbs=st.static_src_rgbs, static_src_cameras=st.static_src_cameras,
                             static_src_masks=st.static_src_masks, uv_grid=sc.uv_grid())
    return dict(self._all)

  def random_sample(self, N_rand, sample_mode, center_ratio=0.8):
    raise NotImplementedError('an evaluation view is rendered whole: get_all()')
