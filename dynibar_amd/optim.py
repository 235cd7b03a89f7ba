"""The optimizer step of the reference's training loop (train.py:199, :467 ``model.optimizer.step()``; ibrnet/model.py:341-364) on one gfx950 kernel.

    self.optimizer = torch.optim.Adam([...six groups...])   ->   self.optimizer = dynibar_amd.optim.Adam([...six groups...])

``Adam`` is a ``torch.optim.Optimizer``: param groups, per-parameter state (``step`` a float32 scalar tensor on the host, ``exp_avg`` and
``exp_avg_sq`` like the parameter), ``state_dict`` / ``load_state_dict`` / ``add_param_group`` and the learning-rate schedulers are torch's, and
a checkpoint's ``'optimizer'`` entry moves between this class and ``torch.optim.Adam`` in both directions (an integer ``step`` as torch 1.10
saved it included).  What differs is ``step()``: ONE launch of ``k_adam_step`` (csrc/dyn_optim.h) updates every tensor of every group, after at
most one pinned, asynchronous host-to-device copy of the per-tensor records -- no device-to-host copy, no synchronisation, no device
allocation after the first step, all on the current stream.

The arithmetic is a contract (include/dynibar_hip.h), fp32 with every operation rounded once:
    m = m + c1 (g - m)      v = v beta2 + (c2 g) g      denom = sqrt(v) / s2 + eps      p = p + (a m) / denom
c1 = fp32(1 - beta1), c2 = fp32(1 - beta2), s2 = fp32(sqrt(1 - beta2^t)), a = fp32(-lr / (1 - beta1^t)) with t the tensor's own step count after
its increment; the scalars are formed here in Python double, as torch forms them, and rounded once.  As with torch a parameter whose
``.grad`` is None is skipped and its step count does not advance, a first-seen parameter starts from zero moments, and a group with lr = 0
still updates its moments.  ``step(zero_grads=True)`` also clears the gradients in the same launch; a following
``zero_grad(set_to_none=False)`` then has nothing left to do.

The guard of a long run: ``step(max_grad_norm=1.0, skip_nonfinite=True)`` is three launches -- ``k_grad_sumsq`` and ``k_grad_stats`` form the global
L2 norm of every gradient of every group (double sums in a fixed order), the clip factor ``coef = min(1, max_grad_norm / (norm + 1e-6))`` of
``torch.nn.utils.clip_grad_norm_`` and whether every gradient element is finite; ``k_adam_step_guarded`` then updates with ``g * coef``, or with
``skip_nonfinite`` leaves p, exp_avg and exp_avg_sq untouched when one is not (``zero_grads`` still clears).  Still one host-to-device copy,
nothing back, no synchronisation, no allocation after the first step; ``.grad`` is never rewritten with the clipped values.  The arithmetic
is a contract as well (include/dynibar_hip.h).  Without the two arguments ``step()`` is the one ``k_adam_step`` launch it always was.
STEP COUNTS: the per-parameter ``step`` lives on the host, and the host cannot know whether the device skipped without a synchronisation, so
``step`` advances for every parameter that had a gradient, skipped or not: a skipped step still counts towards the bias correction.  What
the device saw is in ``opt.grad_stats`` (None before the first guarded step): 0-d device tensor views ``norm``, ``coef``, ``finite``, ``calls``,
``nonfinite`` (and ``sumsq``) into one small buffer that every guarded step overwrites; ``calls`` and ``nonfinite`` count guarded steps and those
whose gradients were not finite since the parameter set last changed.  Reading one (``.item()``) is the caller's synchronisation -- where the
loop prints is the natural place.
``grad_norm(parameters)`` and ``clip_grad_norm_(parameters, max_norm)`` are the same kernels for callers that keep torch's optimizer or want the
scalar alone.

Not built, refused by name: amsgrad, maximize, weight_decay, capturable, differentiable, an explicit foreach / fused.  Tensors must be
contiguous fp32 on ONE HIP device: there is no CPU fallback, host tensors are refused.
"""
from __future__ import annotations

import collections
import ctypes
import inspect
import math
import re

import numpy as np
import torch

from . import _lib
from ._lib import call, params, stream_of

with open(_lib.HEADER) as _f:
  CHUNK = int(re.search(r'#define\s+DYN_ADAM_CHUNK\s+(\d+)', _f.read()).group(1))  # elements per workgroup of k_adam_step

_NP_OF = {ctypes.c_void_p: '<u8', ctypes.c_int64: '<i8', ctypes.c_float: '<f4', ctypes.c_int32: '<i4', ctypes.c_double: '<f8'}
RECORD = np.dtype([(name, _NP_OF[ct]) for name, ct in _lib._STRUCT_SPECS['DynAdamTensor']])
assert RECORD.itemsize == ctypes.sizeof(_lib.STRUCTS['DynAdamTensor']) and RECORD.itemsize % 8 == 0

STATS = np.dtype([(name, _NP_OF[ct]) for name, ct in _lib._STRUCT_SPECS['DynGradStats']])
assert STATS.itemsize == ctypes.sizeof(_lib.STRUCTS['DynGradStats']) == 40 and all(STATS.fields[k][1] % STATS[k].itemsize == 0 for k in STATS.names)

GradStats = collections.namedtuple('GradStats', 'norm coef finite calls nonfinite sumsq')
GradStats.__doc__ = """What the last ``dyn_grad_norm`` over a table wrote (DynGradStats): 0-d device tensors that are VIEWS into the table's buffer."""

_UNBUILT = ('amsgrad', 'maximize', 'capturable', 'differentiable')
_TORCH_HAS_DECOUPLED = 'decoupled_weight_decay' in inspect.signature(torch.optim.Adam.__init__).parameters


def step_scalars(lr, beta1, beta2, t):
  """(a, s2) of the contract for a step count t >= 1: torch's own double arithmetic (``1 - beta ** step``, ``lr / bias_correction1``,
  ``bias_correction2 ** 0.5``), each result rounded to fp32 once."""
  bias_correction1 = 1 - beta1 ** t
  bias_correction2 = 1 - beta2 ** t
  return np.float32(-(lr / bias_correction1)), np.float32(math.sqrt(bias_correction2))


def _chunk_list(sizes):
  return np.concatenate([np.stack([np.full(-(-n // CHUNK), i, np.int32), np.arange(-(-n // CHUNK), dtype=np.int32)], axis=1)
                         for i, n in enumerate(sizes)] or [np.zeros((0, 2), np.int32)])


def _new_tables(dev, sizes):
  """What depends on a parameter set alone: the chunk list (uploaded once), the device buffer its records go to, the partial sums and the
  zeroed DynGradStats of the guard."""
  chunks = _chunk_list(sizes)
  host = torch.from_numpy(np.ascontiguousarray(chunks))
  nbytes = max(1, len(sizes)) * RECORD.itemsize
  if dev.type == 'cuda':
    with torch.cuda.device(dev):
      chunks_dev = host.pin_memory().to(dev, non_blocking=True) if len(chunks) else host.to(dev)
      records_dev = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
      partials = torch.empty((max(1, len(chunks)),), dtype=torch.float64, device=dev)
      stats = torch.zeros((STATS.itemsize // 8,), dtype=torch.int64, device=dev)
  else:  # (the emulator build of the tests: the "device" is the host)
    chunks_dev, records_dev = host, None
    partials = torch.empty((max(1, len(chunks)),), dtype=torch.float64)
    stats = torch.zeros((STATS.itemsize // 8,), dtype=torch.int64)
  f32, i32 = stats.view(torch.float32), stats.view(torch.int32)
  at = {k: STATS.fields[k][1] for k in STATS.names}
  views = GradStats(norm=f32[at['norm'] // 4], coef=f32[at['coef'] // 4], finite=i32[at['finite'] // 4], calls=stats[at['calls'] // 8],
                    nonfinite=stats[at['nonfinite'] // 8], sumsq=stats.view(torch.float64)[at['sumsq'] // 8])
  return dict(device=dev, sizes=sizes, n_chunks=int(len(chunks)), chunks=chunks_dev, records=records_dev, nbytes=nbytes, partials=partials,
              stats=stats, grad_stats=views)


def _stage_in(staging, dev, nbytes):
  """A host buffer for the records that no earlier copy still reads: pinned, with the event of its last copy."""
  if dev.type != 'cuda':
    if not staging:
      staging.append((torch.empty((nbytes,), dtype=torch.uint8), None))
    return staging[0]
  for buf, ev in staging:
    if ev.query():
      return buf, ev
  entry = (torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
  staging.append(entry)
  return entry


def _send(tab, host, event, dev):
  """The records of this call to the device, asynchronously on the current stream -> the tensor the kernels read them from."""
  if dev.type != 'cuda':
    return host
  with torch.cuda.device(dev):
    tab['records'].copy_(host, non_blocking=True)
    event.record(torch.cuda.current_stream(dev))
  return tab['records']


def _check_max_norm(value, who, what):
  if isinstance(value, torch.Tensor):
    raise ValueError(f'{who}: {what} must be a number, a tensor {what} is not built')
  value = float(value)
  if not (math.isfinite(value) and value > 0.0):
    raise ValueError(f'{who}: {what} must be a finite number above 0, got {value}')
  return value


def _name(gi, pi, p):
  return f'parameter {pi} of group {gi} {tuple(p.shape)}'


class Adam(torch.optim.Optimizer):
  """``torch.optim.Adam(params, lr, betas, eps)`` with the whole update in one HIP launch (module docstring)."""

  def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
               capturable=False, differentiable=False, fused=None):
    if isinstance(lr, torch.Tensor):
      raise ValueError('dynibar_amd.optim.Adam: lr must be a number, a tensor lr is not built')
    if not 0.0 <= lr:
      raise ValueError(f'Invalid learning rate: {lr}')
    if not 0.0 <= eps:
      raise ValueError(f'Invalid epsilon value: {eps}')
    if not 0.0 <= betas[0] < 1.0:
      raise ValueError(f'Invalid beta parameter at index 0: {betas[0]}')
    if not 0.0 <= betas[1] < 1.0:
      raise ValueError(f'Invalid beta parameter at index 1: {betas[1]}')
    if foreach is not None or fused is not None:
      raise NotImplementedError('dynibar_amd.optim.Adam: foreach / fused choose among torch\'s implementations; this optimizer has one kernel')
    defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                    capturable=capturable, differentiable=differentiable, fused=None)
    if _TORCH_HAS_DECOUPLED:
      defaults['decoupled_weight_decay'] = False
    self._tables = None     # what depends on the parameter set alone: sizes, the chunk list on the device, the device buffer of the records
    self._staging = []      # pinned host buffers of the records with the event of their last copy
    self._cleared = {}      # id(parameter) -> (gradient tensor, its version) as the last step(zero_grads=True) left it
    self._grad_stats = None  # the views into the tables' DynGradStats, once a guarded step has written them
    super().__init__(params, defaults)

  # ---- torch's layout of groups and state ------------------------------------------------------------------------------------------
  @staticmethod
  def _check_group(group, gi):
    for opt in _UNBUILT:
      if group.get(opt, False):
        raise NotImplementedError(f'dynibar_amd.optim.Adam: {opt}=True (group {gi}) is not built')
    if group.get('weight_decay', 0) != 0:
      raise NotImplementedError(f'dynibar_amd.optim.Adam: weight_decay={group["weight_decay"]} (group {gi}) is not built; the reference trains with 0')
    if group.get('foreach') is not None or group.get('fused') is not None:
      raise NotImplementedError(f'dynibar_amd.optim.Adam: foreach / fused (group {gi}) choose among torch\'s implementations; this optimizer has one kernel')
    if isinstance(group['lr'], torch.Tensor):
      raise ValueError(f'dynibar_amd.optim.Adam: lr of group {gi} must be a number, a tensor lr is not built')

  def add_param_group(self, param_group):
    super().add_param_group(param_group)
    self._check_group(self.param_groups[-1], len(self.param_groups) - 1)
    self._tables = None
    self._grad_stats = None

  def __setstate__(self, state):
    super().__setstate__(state)
    self.__dict__.setdefault('_staging', [])
    self.__dict__.setdefault('_cleared', {})
    self._tables = None
    self._grad_stats = None
    for group in self.param_groups:
      for key, value in (('amsgrad', False), ('maximize', False), ('foreach', None), ('capturable', False), ('differentiable', False),
                         ('fused', None)) + ((('decoupled_weight_decay', False),) if _TORCH_HAS_DECOUPLED else ()):
        group.setdefault(key, value)
      for p in group['params']:
        st = self.state.get(p, [])
        if len(st) != 0 and not torch.is_tensor(st['step']):  # torch <= 1.11 kept a Python int (torch.optim.Adam.__setstate__)
          st['step'] = torch.tensor(float(st['step']), dtype=torch.float32)

  def zero_grad(self, set_to_none=True):
    """torch's, except that ``set_to_none=False`` does not clear again what ``step(zero_grads=True)`` has cleared and nothing has written since."""
    if set_to_none or not self._cleared:
      self._cleared = {}
      return super().zero_grad(set_to_none=set_to_none)
    for group in self.param_groups:
      for p in group['params']:
        g = p.grad
        if g is None:
          continue
        if g.grad_fn is not None:
          g.detach_()
        else:
          g.requires_grad_(False)
        seen = self._cleared.get(id(p))
        if seen is None or seen[0] is not g or seen[1] != g._version:
          g.zero_()

  # ---- the step ------------------------------------------------------------------------------------------------------------------------
  def _collect(self):
    """Every check that can refuse, before anything is changed or launched -> (device, [(group index, parameter, gradient or None)])."""
    entries, dev = [], None
    for gi, group in enumerate(self.param_groups):
      self._check_group(group, gi)
      for pi, p in enumerate(group['params']):
        if p.dtype != torch.float32:
          raise TypeError(f'dynibar_amd.optim.Adam: {_name(gi, pi, p)} is {str(p.dtype).replace("torch.", "")}; the kernel updates float32 only')
        if p.is_sparse or p.layout != torch.strided:
          raise RuntimeError(f'dynibar_amd.optim.Adam: {_name(gi, pi, p)} is not a dense tensor')
        if not p.is_contiguous():
          raise ValueError(f'dynibar_amd.optim.Adam: {_name(gi, pi, p)} is not contiguous')
        if p.numel() >= 2 ** 31:
          raise ValueError(f'dynibar_amd.optim.Adam: {_name(gi, pi, p)} has {p.numel()} elements (below 2^31 per tensor)')
        g = p.grad
        if g is not None:
          if g.is_sparse or g.layout != torch.strided:
            raise RuntimeError(f'dynibar_amd.optim.Adam: the gradient of {_name(gi, pi, p)} is sparse; sparse gradients are not built')
          if g.dtype != torch.float32:
            raise TypeError(f'dynibar_amd.optim.Adam: the gradient of {_name(gi, pi, p)} is {str(g.dtype).replace("torch.", "")}, not float32')
          if g.shape != p.shape or g.device != p.device:
            raise ValueError(f'dynibar_amd.optim.Adam: the gradient of {_name(gi, pi, p)} is {tuple(g.shape)} on {g.device}, '
                             f'its parameter is on {p.device}')
          st = self.state.get(p)
          if st:
            for key in ('exp_avg', 'exp_avg_sq'):
              m = st[key]
              if m.dtype != torch.float32 or m.shape != p.shape or m.device != p.device or not m.is_contiguous():
                raise ValueError(f'dynibar_amd.optim.Adam: {key} of {_name(gi, pi, p)} must be contiguous float32 {tuple(p.shape)} on {p.device}, '
                                 f'got {str(m.dtype).replace("torch.", "")} {tuple(m.shape)} on {m.device}')
        entries.append((gi, p, g))
    for gi, group in enumerate(self.param_groups):  # where the tensors are, after what they are
      for pi, p in enumerate(group['params']):
        if _lib._REQUIRE_DEVICE and not p.is_cuda:
          raise RuntimeError(f'dynibar_amd.optim.Adam needs parameters on a HIP device (cuda:N), there is no CPU fallback; {_name(gi, pi, p)} is on {p.device}')
        if dev is None:
          dev = p.device
        elif p.device != dev:
          raise RuntimeError(f'dynibar_amd.optim.Adam: parameters on more than one device: {_name(gi, pi, p)} is on {p.device}, others on {dev} (one HIP device)')
    return dev, entries

  def _make_tables(self, dev, sizes):
    """The chunk list of a parameter set (uploaded once), the device buffer its records go to and the guard's buffers."""
    self._staging = []
    self._grad_stats = None
    self._tables = _new_tables(dev, sizes)

  def _stage(self, dev, nbytes):
    return _stage_in(self._staging, dev, nbytes)

  @property
  def grad_stats(self):
    """``GradStats`` of the last guarded step (device tensor views; reading one synchronises), None before the first."""
    return self.__dict__.get('_grad_stats')

  @torch.no_grad()
  def step(self, closure=None, zero_grads=False, max_grad_norm=None, skip_nonfinite=False):
    """One ``k_adam_step`` launch over every parameter that has a gradient.  zero_grads: the launch also stores 0 to the gradients it read.
    max_grad_norm (a finite number above 0) and / or skip_nonfinite: the guarded step of the module docstring, three launches."""
    guarded = max_grad_norm is not None or bool(skip_nonfinite)
    if max_grad_norm is not None:
      max_grad_norm = _check_max_norm(max_grad_norm, 'dynibar_amd.optim.Adam', 'max_grad_norm')
    loss = None
    if closure is not None:
      with torch.enable_grad():
        loss = closure()
    dev, entries = self._collect()
    self._cleared = {}
    if dev is None or all(g is None for _, _, g in entries):
      return loss
    sizes = [p.numel() for _, p, _ in entries]
    if self._tables is None or self._tables['device'] != dev or self._tables['sizes'] != sizes:
      self._make_tables(dev, sizes)
    tab = self._tables
    if tab['n_chunks'] == 0:
      return loss
    n = len(entries)
    ptr = {k: [0] * n for k in 'pgmv'}
    a, s2, c1, c2, b2, ep = ([0.0] * n for _ in range(6))
    skip = [1] * n
    scalars, copies, cleared = {}, [], {}
    for i, (gi, p, g) in enumerate(entries):
      if g is None or sizes[i] == 0:
        continue
      group = self.param_groups[gi]
      st = self.state[p]
      if len(st) == 0:  # torch's layout of a first-seen parameter
        st['step'] = torch.tensor(0.0, dtype=torch.float32)
        st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
      st['step'] += 1
      lr, (beta1, beta2), eps = group['lr'], group['betas'], group['eps']
      key = (lr, beta1, beta2, st['step'].item())
      if key not in scalars:
        scalars[key] = step_scalars(*key)
      gc = g if g.is_contiguous() else g.contiguous()
      if gc is not g:
        copies.append((g, gc))  # (kept alive until the launch is enqueued; cleared below when the kernel clears its copy)
      ptr['p'][i], ptr['g'][i], ptr['m'][i], ptr['v'][i] = p.data_ptr(), gc.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr()
      a[i], s2[i] = scalars[key]
      c1[i], c2[i], b2[i], ep[i] = 1 - beta1, 1 - beta2, beta2, eps
      skip[i] = 0
      if zero_grads:
        cleared[id(p)] = g
    host, event = self._stage(dev, tab['nbytes'])
    rec = host.numpy()[:n * RECORD.itemsize].view(RECORD)
    for k in 'pgmv':
      rec[k] = ptr[k]
    rec['n'], rec['a'], rec['s2'], rec['c1'], rec['c2'], rec['beta2'], rec['eps'], rec['skip'], rec['reserved'] = sizes, a, s2, c1, c2, b2, ep, skip, 0
    records = _send(tab, host, event, dev)
    like = entries[0][1]
    table = dict(tensors=ctypes.c_void_p(records.data_ptr()), n_tensors=n, chunks=ctypes.c_void_p(tab['chunks'].data_ptr()), n_chunks=tab['n_chunks'])
    if guarded:
      stats = ctypes.c_void_p(tab['stats'].data_ptr())
      call('dyn_grad_norm', params('DynGradNormParams', partials=ctypes.c_void_p(tab['partials'].data_ptr()), stats=stats,
                                   max_norm=0.0 if max_grad_norm is None else max_grad_norm, count=1, **table), stream_of(like))
      call('dyn_adam_step_guarded', params('DynAdamGuardedParams', zero_grads=1 if zero_grads else 0, skip_nonfinite=1 if skip_nonfinite else 0,
                                           stats=stats, **table), stream_of(like))
      self._grad_stats = tab['grad_stats']
    else:
      call('dyn_adam_step', params('DynAdamParams', zero_grads=1 if zero_grads else 0, **table), stream_of(like))
    if zero_grads:
      for g, _ in copies:  # the kernel cleared the contiguous copy, not the strided gradient itself
        g.zero_()
      self._cleared = {k: (g, g._version) for k, g in cleared.items()}
    return loss


# ---- the norm and the clip on their own ----------------------------------------------------------------------------------------------
_TABLES = collections.OrderedDict()  # (device, sizes) -> tables and their staging buffers, for grad_norm / clip_grad_norm_
_TABLES_KEPT = 8
_NONFINITE = ('The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be clipped. To disable this error and scale '
              'the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`')


def _gradients(parameters, who):
  """-> (device, [gradient]) of the parameters that have one, after every check that can refuse"""
  if isinstance(parameters, torch.Tensor):
    parameters = [parameters]
  grads, dev = [], None
  for i, p in enumerate(parameters):
    g = p.grad
    if g is None:
      continue
    if g.is_sparse or g.layout != torch.strided:
      raise RuntimeError(f'{who}: the gradient of parameter {i} {tuple(p.shape)} is sparse; sparse gradients are not built')
    if g.dtype != torch.float32:
      raise TypeError(f'{who}: the gradient of parameter {i} {tuple(p.shape)} is {str(g.dtype).replace("torch.", "")}, not float32')
    if g.numel() >= 2 ** 31:
      raise ValueError(f'{who}: the gradient of parameter {i} has {g.numel()} elements (below 2^31 per tensor)')
    if _lib._REQUIRE_DEVICE and not g.is_cuda:
      raise RuntimeError(f'{who} needs gradients on a HIP device (cuda:N), there is no CPU fallback; that of parameter {i} is on {g.device}')
    if dev is None:
      dev = g.device
    elif g.device != dev:
      raise RuntimeError(f'{who}: gradients on more than one device: that of parameter {i} is on {g.device}, others on {dev} (one HIP device)')
    grads.append(g)
  return dev, grads


def _norm_of(grads, dev, max_norm):
  """dyn_grad_norm over the gradients -> (tables, the call's table fields, [(strided gradient, its contiguous copy)])"""
  sizes = [g.numel() for g in grads]
  key = (str(dev), tuple(sizes))
  tab = _TABLES.get(key)
  if tab is None:
    tab = _TABLES[key] = dict(_new_tables(dev, sizes), staging=[])
    while len(_TABLES) > _TABLES_KEPT:
      _TABLES.popitem(last=False)
  else:
    _TABLES.move_to_end(key)
  n, copies = len(grads), []
  host, event = _stage_in(tab['staging'], dev, tab['nbytes'])
  rec = host.numpy()[:n * RECORD.itemsize].view(RECORD)
  rec[:] = 0
  for i, g in enumerate(grads):
    gc = g if g.is_contiguous() else g.contiguous()
    if gc is not g:
      copies.append((g, gc))
    rec['g'][i], rec['n'][i], rec['skip'][i] = gc.data_ptr(), sizes[i], 1 if sizes[i] == 0 else 0
  records = _send(tab, host, event, dev)
  table = dict(tensors=ctypes.c_void_p(records.data_ptr()), n_tensors=n, chunks=ctypes.c_void_p(tab['chunks'].data_ptr()), n_chunks=tab['n_chunks'])
  call('dyn_grad_norm', params('DynGradNormParams', partials=ctypes.c_void_p(tab['partials'].data_ptr()),
                               stats=ctypes.c_void_p(tab['stats'].data_ptr()), max_norm=max_norm, count=1, **table), stream_of(grads[0]))
  return tab, table, copies


@torch.no_grad()
def grad_norm(parameters):
  """The global L2 norm of the ``.grad`` of every parameter that has one: a 0-d fp32 tensor on their device, by ``k_grad_sumsq`` and ``k_grad_stats``
  (the contract of include/dynibar_hip.h: what ``Adam.step(max_grad_norm=...)`` leaves in ``opt.grad_stats.norm`` for the same gradients, bit for
  bit).  Nothing is read back and nothing synchronises; the result is the caller's own (a 4-byte device copy out of the cached table).
  No gradients at all: a zero."""
  dev, grads = _gradients(parameters, 'dynibar_amd.optim.grad_norm')
  if not grads or sum(g.numel() for g in grads) == 0:
    return torch.zeros((), dtype=torch.float32, device=dev)
  tab, _, _ = _norm_of(grads, dev, 0.0)
  return tab['grad_stats'].norm.clone()


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
  """``torch.nn.utils.clip_grad_norm_`` for the L2 norm in three launches: the norm as ``grad_norm`` forms it, then ``k_grad_scale`` multiplies every
  ``.grad`` in place by ``coef = min(1, max_norm / (norm + 1e-6))`` (nothing is written when coef is 1).  Returns the norm.  Gradients that are not
  finite leave coef at 1: the gradients stay as they are, where torch would turn all of them into NaN.  ``error_if_nonfinite=True`` reads the
  result back -- the one synchronisation here -- and raises torch's RuntimeError before anything is scaled."""
  who = 'dynibar_amd.optim.clip_grad_norm_'
  if float(norm_type) != 2.0:
    raise NotImplementedError(f'{who}: norm_type={norm_type} is not built, only the L2 norm is')
  if foreach is not None:
    raise NotImplementedError(f'{who}: foreach chooses among torch\'s implementations; this one has its own kernels')
  max_norm = _check_max_norm(max_norm, who, 'max_norm')
  dev, grads = _gradients(parameters, who)
  if not grads or sum(g.numel() for g in grads) == 0:
    return torch.zeros((), dtype=torch.float32, device=dev)
  tab, table, copies = _norm_of(grads, dev, max_norm)
  views = tab['grad_stats']
  if error_if_nonfinite:
    seen = tab['stats'].cpu().numpy().view(STATS)[0]
    if not seen['finite'] or not math.isfinite(float(seen['norm'])):
      raise RuntimeError(_NONFINITE)
  call('dyn_grad_scale', params('DynGradScaleParams', stats=ctypes.c_void_p(tab['stats'].data_ptr()), **table), stream_of(grads[0]))
  for g, _ in copies:  # the kernel scaled the contiguous copy, not the strided gradient itself: the same single fp32 product by a torch op
    g.mul_(views.coef)
  return views.norm.clone()
