"""The training objective of the reference's monocular main loop (train.py:300-456) and ``eff_distloss_native``, on the gfx950 kernels.

    from torch_efficient_distloss import eff_distloss_native   ->   from dynibar_amd.objective import eff_distloss_native

    objective = MonoObjective(args)                      # once, next to rgb_criterion = Criterion()
    loss, logged = objective(ret, ray_batch, epoch)      # replaces train.py:300-456
    loss.backward()
    scalars_to_log.update(zip(LOGGED, logged.tolist()))  # ONE device-to-host copy instead of seven .item() calls

``ret`` is the dictionary ``render_rays_mono(is_train=True)`` returns.  The eight terms -- colour (``Criterion``, temporal, the dynamic-only
term while ``epoch < init_decay_epoch``, the two ``_dy`` terms decayed by ``10 ** divisor``), disparity, flow, trajectory consistency
(``anneal_cycle`` / ``cycle_factor``), the three scene-flow regularisers, skew entropy, distortion and the adaptive static term with its
``divisor > 4`` addition -- are computed by ``dyn_objective_fwd`` (csrc/dyn_objective.h): three launches, per-workgroup partial sums added in a
fixed order, no float atomics, so ``loss``, ``logged`` and every cotangent are bitwise reproducible.  ``dyn_objective_bwd`` is two launches and
reads ``grad_loss`` from device memory.  Neither direction synchronises or reads a value back.

``logged`` is one detached device tensor in the order ``LOGGED``; ``loss`` is a 0-d tensor that carries the graph.  What the reference detaches
stays detached (``occ_weights``, ``occ_weight_map``, the ``1 - weights_ratio`` factor of the static mask and its ``< 0.1`` mask); an ``occ_*``
input that carries a graph is an error.  Inputs that do not require a gradient, or that the selected terms do not reach, get none computed or
allocated.  Conventions as torch has them: ``sign(0) = 0``, ``clamp(min=c)`` passes the gradient where ``x >= c``.

Limits (``ValueError``): ``S >= 2``, at most 6 flow views, fp32 tensors on a HIP device, boolean ``mask`` entries (what the renderer returns).
There is no eager fallback.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import call, params, stream_of
from .train_static import POISON_SCRATCH

LOGGED = ('loss', 'rgb', 'cycle', 'flow', 'disp', 'reg', 'entropy', 'distortion', 'static')
ALL = ('rgb', 'disp', 'flow', 'cycle', 'reg', 'entropy', 'distortion', 'static')  # the names tests/cases.py:MONO_TRAIN_LOSSES uses

# the tensors of one call, in the order the autograd Function takes them: the differentiable ones first
_DIFF = ('rgb_ref', 'rgb_dy', 'rgb_static', 'rgb_ref_dy', 'rgb_anc', 'rgb_anc_dy', 'depth', 'render_flows', 'weights', 'weights_dy', 'weights_st',
         'pts_traj_ref', 'pts_traj_anchor', 'sf_seq')
_MASKS = ('mask_ref', 'mask_ref_dy', 'mask_anc', 'mask_anc_dy')
_CONST = ('s_vals',) + _MASKS + ('owm_anc', 'owm_anc_dy', 'occ_weights', 't_rgb', 't_disp', 't_flows', 't_masks', 'motion_mask', 'static_mask')
_NAMES = _DIFF + _CONST
# which weight of DynObjectiveParams reaches which cotangent: a zero weight means the term is left out and the input gets None
_REACH = dict(rgb_ref=('k_rgb',), rgb_dy=('k_rgb_dyn',), rgb_static=('k_static',), rgb_ref_dy=('k_rgb_dy',), rgb_anc=('k_rgb',),
              rgb_anc_dy=('k_rgb_dy',), depth=('w_disp',), render_flows=('w_flow',), weights=('w_distortion',),
              weights_dy=('w_entropy', 'k_static2'), weights_st=('w_entropy',), pts_traj_ref=('w_cycle',), pts_traj_anchor=('w_cycle',),
              sf_seq=('w_reg',))


def _dptr(t):
  """device pointer of a tensor whose last dimension has unit stride (rows may be strided); None -> NULL"""
  import ctypes
  if t is None:
    return None
  if _lib._REQUIRE_DEVICE and not t.is_cuda:
    raise ValueError('dynibar_amd.objective needs tensors on a HIP device (cuda:N); got ' + str(t.device))
  return ctypes.c_void_p(t.data_ptr())


def _scratch(n, dtype, device):
  t = torch.empty((n,), dtype=dtype, device=device)
  if POISON_SCRATCH:  # (train_static.py) under test the kernels must fill what they later read
    t.fill_(float('nan')) if dtype.is_floating_point else t.fill_(0xFF)
  return t


def _f32(t, what):
  if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
    raise ValueError(f'{what} must be a float32 tensor, got {getattr(t, "dtype", type(t))}')
  return t


# ---- eff_distloss_native ---------------------------------------------------------------------------------------------------------------
def _rows(t, S):
  """[..., S] -> a [R, S] view with unit stride along S and its row stride (a slice such as weights[:, :-1] is used in place)"""
  if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= S:
    return t, t.stride(0)
  t = t.reshape(-1, S).contiguous()
  return t, S


class _DistLoss(torch.autograd.Function):

  @staticmethod
  def forward(ctx, w, m, interval):
    S = w.shape[-1]
    R = w.numel() // S
    wr, ld_w = _rows(w, S)
    mr, ld_m = _rows(m, S)
    ir, ld_i = _rows(interval, S)
    part = _scratch(int(_lib.lib().dyn_distloss_partials(R)), torch.float64, w.device)
    loss = torch.empty((), dtype=torch.float32, device=w.device)
    call('dyn_distloss_fwd', _dptr(wr), ld_w, _dptr(mr), ld_m, _dptr(ir), ld_i, R, S, _dptr(part), _dptr(loss), stream_of(w))
    ctx.save_for_backward(w, m, interval)
    return loss

  @staticmethod
  def backward(ctx, g):
    w, m, interval = ctx.saved_tensors
    S = w.shape[-1]
    R = w.numel() // S
    wr, ld_w = _rows(w, S)
    mr, ld_m = _rows(m, S)
    ir, ld_i = _rows(interval, S)
    out = [torch.empty(w.shape, dtype=torch.float32, device=w.device) if need else None for need in ctx.needs_input_grad]
    g = g.contiguous().float()
    call('dyn_distloss_bwd', _dptr(wr), ld_w, _dptr(mr), ld_m, _dptr(ir), ld_i, R, S, _dptr(g), _dptr(out[0]), _dptr(out[1]), _dptr(out[2]),
         stream_of(w))
    return tuple(out)


def eff_distloss_native(w, m, interval):
  """torch_efficient_distloss.eff_distloss_native(w, m, interval): the O(S) form of the mip-NeRF-360 distortion loss, mean over the rays.
  w [..., S] sample weights, m [..., S] interval midpoints, interval [..., S] interval lengths (or one number).  Gradients to w and, where
  they require one, to m and interval."""
  _f32(w, 'w')
  if w.dim() < 1 or w.shape[-1] < 1 or w.numel() == 0:
    raise ValueError(f'w must be [..., S] with S >= 1, got {tuple(w.shape)}')
  if not isinstance(interval, torch.Tensor):
    interval = torch.full((), float(interval), dtype=torch.float32, device=w.device)
  m, interval = _f32(m, 'm').expand(w.shape), _f32(interval, 'interval').expand(w.shape)
  return _DistLoss.apply(w, m, interval)


# ---- the main loop's objective -----------------------------------------------------------------------------------------------------------
def _params(t, cfg, ws):
  R, S = t['weights'].shape
  kw = {k: _dptr(t[k]) for k in _NAMES if k not in ('pts_traj_ref', 'pts_traj_anchor', 'sf_seq')}
  cyc = cfg['w_cycle'] != 0.0
  kw.update(pts_traj_ref=_dptr(t['pts_traj_ref']) if cyc else None, pts_traj_anchor=_dptr(t['pts_traj_anchor']) if cyc else None,
            sf_seq=_dptr(t['sf_seq']) if cfg['w_reg'] != 0.0 else None)
  return params('DynObjectiveParams', R=R, S=S, T=cfg['T'], NV=cfg['NV'], workspace=_dptr(ws), workspace_bytes=ws.numel(),
                **{k: cfg[k] for k in _WEIGHTS}, **kw)


_WEIGHTS = ('k_rgb', 'k_rgb_dyn', 'k_rgb_dy', 'w_disp', 'w_flow', 'w_cycle', 'w_reg', 'w_entropy', 'w_distortion', 'k_static', 'k_static2')


class _MonoObjectiveFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, cfg, *tensors):
    t = dict(zip(_NAMES, tensors))
    R, S = t['weights'].shape
    dev = t['weights'].device
    need = int(_lib.lib().dyn_objective_workspace_bytes(R, S))
    if need == 0:
      raise ValueError(f'objective of R={R} S={S} is unsupported (S >= 2, R * S <= 2^28)')
    ws = _scratch(need // 8, torch.float64, dev).view(torch.uint8)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    logged = torch.empty((len(LOGGED),), dtype=torch.float32, device=dev)
    call('dyn_objective_fwd', _params(t, cfg, ws), _dptr(loss), _dptr(logged), stream_of(t['weights']))
    ctx.cfg = cfg
    ctx.save_for_backward(ws, *tensors)
    ctx.mark_non_differentiable(logged)
    ctx.set_materialize_grads(False)  # (no zeros tensor for the cotangent of `logged`)
    return loss, logged

  @staticmethod
  def backward(ctx, g, _g_logged):
    cfg = ctx.cfg
    ws, tensors = ctx.saved_tensors[0], ctx.saved_tensors[1:]
    t = dict(zip(_NAMES, tensors))
    grads = {}
    for i, k in enumerate(_DIFF if g is not None else ()):  # (input 0 of the Function is cfg)
      if ctx.needs_input_grad[1 + i] and any(cfg[w] != 0.0 for w in _REACH[k]) and t[k].numel() > 0:
        grads[k] = torch.empty(t[k].shape, dtype=torch.float32, device=t[k].device)
    if grads and g is not None:
      g = g.contiguous().float()
      gp = params('DynObjectiveGrads', grad_loss=_dptr(g), **{k: _dptr(v) for k, v in grads.items()})
      call('dyn_objective_bwd', _params(t, cfg, ws), gp, stream_of(t['weights']))
    return (None,) + tuple(grads.get(k) for k in _DIFF) + (None,) * len(_CONST)


class MonoObjective:
  """``MonoObjective(args)(ret, ray_batch, epoch, terms=ALL) -> (loss, logged)``: train.py:300-456 on the HIP kernels (module docstring).
  args: w_disp, w_flow, w_cycle, w_reg, w_skew_entropy, w_distortion, decay_rate, init_decay_epoch, anneal_cycle, cycle_factor.
  terms: a subset of ``ALL``, each with its train.py weight; a term left out logs 0 and reaches no input."""

  def __init__(self, args):
    g = lambda k: getattr(args, k)
    self.w_disp, self.w_flow, self.w_cycle, self.w_reg = float(g('w_disp')), float(g('w_flow')), float(g('w_cycle')), float(g('w_reg'))
    self.w_skew_entropy, self.w_distortion = float(g('w_skew_entropy')), float(g('w_distortion'))
    self.decay_rate, self.init_decay_epoch = float(g('decay_rate')), int(g('init_decay_epoch'))
    self.anneal_cycle, self.cycle_factor = bool(g('anneal_cycle')), float(g('cycle_factor'))
    if self.init_decay_epoch <= 0:
      raise ValueError('init_decay_epoch must be positive')

  def schedule(self, epoch, terms=ALL):
    """the weights of DynObjectiveParams at `epoch` (train.py:302, :309, :318-331, :345, :354-357, :420, :437-441)"""
    unknown = set(terms) - set(ALL)
    if unknown:
      raise ValueError(f'unknown terms {sorted(unknown)}: choose from {ALL}')
    on = lambda name, v: float(v) if name in terms else 0.0
    divisor = epoch // self.init_decay_epoch
    w_cycle = min(0.5, self.w_cycle + divisor * self.cycle_factor) if self.anneal_cycle else self.w_cycle
    return dict(k_rgb=on('rgb', 1.0), k_rgb_dyn=on('rgb', 1.0 if epoch < self.init_decay_epoch else 0.0), k_rgb_dy=on('rgb', 1.0 / (10.0 ** divisor)),
                w_disp=on('disp', self.w_disp / (self.decay_rate ** divisor)), w_flow=on('flow', self.w_flow / (self.decay_rate ** divisor)),
                w_cycle=on('cycle', w_cycle), w_reg=on('reg', self.w_reg), w_entropy=on('entropy', self.w_skew_entropy),
                w_distortion=on('distortion', self.w_distortion), k_static=on('static', 1.0), k_static2=on('static', 0.1 if divisor > 4 else 0.0))

  def __call__(self, ret, ray_batch, epoch, terms=ALL):
    cfg = self.schedule(int(epoch), tuple(terms))
    ref, anc = ret['outputs_coarse_ref'], ret['outputs_coarse_anchor']
    ref_dy, anc_dy = ret['outputs_coarse_ref_dy'], ret['outputs_coarse_anchor_dy']
    t = dict(rgb_ref=ref['rgb'], rgb_dy=ref['rgb_dy'], rgb_static=ref['rgb_static'], rgb_ref_dy=ref_dy['rgb'], rgb_anc=anc['rgb'],
             rgb_anc_dy=anc_dy['rgb'], depth=ref['depth'], render_flows=ref['render_flows'], weights=ref['weights'], weights_dy=ref['weights_dy'],
             weights_st=ref['weights_st'], pts_traj_ref=anc['pts_traj_ref'], pts_traj_anchor=anc['pts_traj_anchor'], sf_seq=anc['sf_seq'],
             s_vals=ref['s_vals'], mask_ref=ref['mask'], mask_ref_dy=ref_dy['mask'], mask_anc=anc['mask'], mask_anc_dy=anc_dy['mask'],
             owm_anc=anc['occ_weight_map'], owm_anc_dy=anc_dy['occ_weight_map'], occ_weights=anc['occ_weights'])
    w = _f32(t['weights'], "outputs_coarse_ref['weights']")
    if w.dim() != 2:
      raise ValueError(f"outputs_coarse_ref['weights'] must be [R, S], got {tuple(w.shape)}")
    R, S = w.shape
    dev = w.device
    if _lib._REQUIRE_DEVICE and not w.is_cuda:
      raise ValueError('MonoObjective needs tensors on a HIP device (cuda:N); got ' + str(dev))
    if S < 2:
      raise ValueError(f'S = {S}: the objective needs at least 2 samples per ray (the spatial smoothness term is a mean over S - 1 elements)')
    NV = int(t['render_flows'].shape[0])
    if NV > 6:
      raise ValueError(f'{NV} flow views: render_rays_mono returns at most 6')
    for k in _MASKS:
      if t[k].dtype != torch.bool:
        raise ValueError(f'{k} must be a boolean tensor (what render_rays_mono returns), got {t[k].dtype}')
      t[k] = t[k].contiguous().view(torch.uint8)
    for k in ('owm_anc', 'owm_anc_dy', 'occ_weights', 's_vals'):
      if t[k].requires_grad:
        raise ValueError(f'{k} carries a graph: the reference detaches it (render_ray.py:1216, :1243), and the objective gives it no gradient')
    for k, src in (('t_rgb', 'rgb'), ('t_disp', 'disp'), ('t_flows', 'flows'), ('t_masks', 'masks'), ('motion_mask', 'motion_mask'),
                   ('static_mask', 'static_mask')):
      t[k] = ray_batch[src].to(device=dev, dtype=torch.float32)
    shapes = dict(rgb_ref=(R, 3), rgb_dy=(R, 3), rgb_static=(R, 3), rgb_ref_dy=(R, 3), rgb_anc=(R, 3), rgb_anc_dy=(R, 3), depth=(R,),
                  render_flows=(NV, R, 2), weights_dy=(R, S), weights_st=(R, S), s_vals=(R, S), occ_weights=(R, S), owm_anc=(R,), owm_anc_dy=(R,),
                  mask_ref=(R,), mask_ref_dy=(R,), mask_anc=(R,), mask_anc_dy=(R,), t_rgb=(R, 3), t_disp=(R,), motion_mask=(R,), static_mask=(R,),
                  sf_seq=(6, R, S, 3))
    for k, shp in shapes.items():
      if tuple(t[k].shape) != shp:
        raise ValueError(f'{k} must be {shp}, got {tuple(t[k].shape)}')
    T = int(t['pts_traj_ref'].shape[0])
    for k in ('pts_traj_ref', 'pts_traj_anchor'):
      if tuple(t[k].shape) != (T, R, S, 3):
        raise ValueError(f'{k} must be {(T, R, S, 3)}, got {tuple(t[k].shape)}')
    if t['t_flows'].shape[0] < NV or tuple(t['t_flows'].shape[1:]) != (R, 2) or tuple(t['t_masks'].shape) != (t['t_flows'].shape[0], R, 1):
      raise ValueError(f"ray_batch['flows'] / ['masks'] must be [>={NV}, {R}, 2] / [.., {R}, 1], got {tuple(t['t_flows'].shape)} / {tuple(t['t_masks'].shape)}")
    if T == 0:
      cfg['w_cycle'] = 0.0  # no frame both passes look at: sum over nothing / (0 + 1e-8) = 0 in the reference too
    cfg.update(T=T, NV=NV)
    tensors = []
    for k in _NAMES:
      v = t[k] if k in _MASKS else _f32(t[k], k)
      if v.device != dev:
        raise ValueError(f'{k} is on {v.device}, the weights on {dev}')
      tensors.append(v.contiguous())
    return _MonoObjectiveFn.apply(cfg, *tensors)
