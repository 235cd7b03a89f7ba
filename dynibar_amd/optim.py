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
STEP COUNTS, two behaviours.  ``capturable=False`` (the default): the per-parameter ``step`` lives on the host, and the host cannot know whether
the device skipped without a synchronisation, so ``step`` advances for every parameter that had a gradient, skipped or not: a skipped step
still counts towards the bias correction.  ``capturable=True``: ``step`` is a float32 0-d DEVICE tensor (torch's capturable layout) next to
``beta_pow``, a float64 ``[beta1^t, beta2^t]`` device tensor of ours; the kernel forms the bias corrections from them in double and
``k_adam_advance`` advances both after the step -- unless the step was held, which then leaves p, the moments, ``step`` and ``beta_pow`` bit for
bit as they were: a run with a held step equals the run of its finite steps alone.  (``beta_pow`` is a running product: betas changed in
mid-run continue from it, where torch would form ``beta ** step`` afresh.)  What the device saw is in ``opt.grad_stats`` (None before the first guarded step): 0-d device tensor views ``norm``, ``coef``, ``finite``, ``calls``,
``nonfinite`` (and ``sumsq``) into one small buffer that every guarded step overwrites; ``calls`` and ``nonfinite`` count guarded steps and those
whose gradients were not finite since the parameter set last changed.  Reading one (``.item()``) is the caller's synchronisation -- where the
loop prints is the natural place.
``grad_norm(parameters)`` and ``clip_grad_norm_(parameters, max_norm)`` are the same kernels for callers that keep torch's optimizer or want the
scalar alone.

THE OPTIONS of torch's constructor live in two further classes, ``AdamX`` (``torch.optim.Adam``'s whole constructor) and ``AdamW``
(``torch.optim.AdamW``): ``weight_decay`` (coupled, or decoupled with ``decoupled_weight_decay=True`` / the ``AdamW`` class), ``amsgrad`` (state
``max_exp_avg_sq``), ``maximize`` and ``capturable``.  ``Adam`` itself is what it was: it refuses these four by name and launches the plain kernels.
An ``AdamX`` / ``AdamW`` none of whose groups sets one of them launches ``k_adam_step`` / ``k_adam_step_guarded`` exactly as ``Adam`` does; otherwise every group, whatever its options, goes through ONE launch of the extended kernel
(``dyn_adamx_step`` / ``dyn_adamx_step_guarded``, a record and a contract of their own in include/dynibar_hip.h) plus the one-thread-per-tensor
``k_adam_advance`` when a group is capturable.  Per element: g1 = -g under maximize; g2 = g1 coef under the guard; g3 = g2 + wd p (coupled);
p1 = p decay with decay = fp32(1 - lr weight_decay) (decoupled); m, v as above on g3; vmax = v > vmax ? v : vmax and denom from vmax under
amsgrad (a NaN v leaves vmax alone, the one difference from ``torch.maximum``; ``skip_nonfinite`` keeps NaN out); p = p1 + (a m) / denom.

VISIBILITY: the kernels write the parameters through raw pointers, so after every step each stepped parameter's version counter is advanced
(``torch._C._increment_version``, no launch): the packed inference weights, cached by ``(data_ptr, _version)``, are rebuilt by the next render.

Not built, refused by name: differentiable, an explicit foreach / fused, a tensor lr, sparse gradients (and in ``Adam`` the four options above).  Tensors must be
contiguous fp32 on ONE HIP device: there is no CPU fallback, host tensors are refused.
"""
from __future__ import annotations

import collections
import ctypes
import inspect
import math
import re
import types

import numpy as np
import torch

from . import _lib
from ._lib import call, params, stream_of

with open(_lib.HEADER) as _f:
  CHUNK = int(re.search(r'#define\s+DYN_ADAM_CHUNK\s+(\d+)', _f.read()).group(1))  # elements per workgroup of k_adam_step

_NP_OF = {ctypes.c_void_p: '<u8', ctypes.c_int64: '<i8', ctypes.c_float: '<f4', ctypes.c_int32: '<i4', ctypes.c_double: '<f8'}
RECORD = np.dtype([(name, _NP_OF[ct]) for name, ct in _lib._STRUCT_SPECS['DynAdamTensor']])
assert RECORD.itemsize == ctypes.sizeof(_lib.STRUCTS['DynAdamTensor']) and RECORD.itemsize % 8 == 0

XRECORD = np.dtype([(name, _NP_OF[ct]) for name, ct in _lib._STRUCT_SPECS['DynAdamXTensor']])  # the record of the extended step
assert XRECORD.itemsize == ctypes.sizeof(_lib.STRUCTS['DynAdamXTensor']) == 128 and RECORD.names[:-1] == XRECORD.names[:len(RECORD.names) - 1]

STATS = np.dtype([(name, _NP_OF[ct]) for name, ct in _lib._STRUCT_SPECS['DynGradStats']])
assert STATS.itemsize == ctypes.sizeof(_lib.STRUCTS['DynGradStats']) == 40 and all(STATS.fields[k][1] % STATS[k].itemsize == 0 for k in STATS.names)

GradStats = collections.namedtuple('GradStats', 'norm coef finite calls nonfinite sumsq')
GradStats.__doc__ = """What the last ``dyn_grad_norm`` over a table wrote (DynGradStats): 0-d device tensors that are VIEWS into the table's buffer."""

_UNBUILT = ('differentiable',)
_EXTENDED = ('amsgrad', 'maximize', 'capturable')  # with weight_decay != 0: what sends a step through dyn_adamx_step
_STEP_CALLS = {(False, False): ('dyn_adam_step', 'DynAdamParams'), (False, True): ('dyn_adam_step_guarded', 'DynAdamGuardedParams'),
               (True, False): ('dyn_adamx_step', 'DynAdamXParams'), (True, True): ('dyn_adamx_step_guarded', 'DynAdamXGuardedParams')}  # by (extended, guarded)
_increment_version = getattr(torch._C, '_increment_version', None)
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


def _new_tables(dev, sizes, extended=False):
  """What depends on a parameter set alone: the chunk list (uploaded once), the device buffer its records go to with the rotation of host
  buffers they are staged in, the partial sums and the zeroed DynGradStats of the guard.  extended: the buffers hold the DynAdamTensor
  records (the norm reads them) and behind them the DynAdamXTensor records of the same tensors, so a step is still one copy."""
  chunks = _chunk_list(sizes)
  host = torch.from_numpy(np.ascontiguousarray(chunks))
  nbytes = max(1, len(sizes)) * (RECORD.itemsize + (XRECORD.itemsize if extended else 0))
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
  return dict(device=dev, sizes=sizes, extended=bool(extended), n_chunks=int(len(chunks)), chunks=chunks_dev, records=records_dev, nbytes=nbytes, partials=partials,
              stats=stats, grad_stats=views, staging=[])  # staging: pinned host buffers of the records with the event of their last copy


def _stage_in(tab):
  """A host buffer for the records that no earlier copy still reads: pinned, with the event of its last copy."""
  staging, nbytes = tab['staging'], tab['nbytes']
  if tab['device'].type != 'cuda':
    if not staging:
      staging.append((torch.empty((nbytes,), dtype=torch.uint8), None))
    return staging[0]
  for buf, ev in staging:
    if ev.query():
      return buf, ev
  entry = (torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
  staging.append(entry)
  return entry


def _records(host, pointers, sizes, skip):
  """The first len(sizes) DynAdamTensor rows of a staging buffer from the pointers (field -> one per tensor), the sizes and the skip
  flags; every other field is 0 and the caller's to fill -> the rows"""
  rec = host.numpy()[:len(sizes) * RECORD.itemsize].view(RECORD)
  rec[:] = 0
  for k, column in pointers.items():
    rec[k] = column
  rec['n'], rec['skip'] = sizes, skip
  return rec


def _send(tab, host, event):
  """The records of this call to the device, asynchronously on the current stream -> the call's fields that every entry point takes"""
  dev, records = tab['device'], host
  if dev.type == 'cuda':
    records = tab['records']
    with torch.cuda.device(dev):
      records.copy_(host, non_blocking=True)
      event.record(torch.cuda.current_stream(dev))
  return dict(tensors=ctypes.c_void_p(records.data_ptr()), n_tensors=len(tab['sizes']), chunks=ctypes.c_void_p(tab['chunks'].data_ptr()),
              n_chunks=tab['n_chunks'])


def _contiguous(g, copies):
  """A contiguous copy of a strided g, with (g, copy) remembered: what a kernel writes to the copy, the caller owes the original."""
  copies.append((g, g.contiguous()))
  return copies[-1][1]


def _check_gradient(g, who, name, *args):
  """What every entry point refuses about a gradient itself; name(*args) names its parameter in the caller's words."""
  if g.is_sparse or g.layout != torch.strided:
    raise RuntimeError(f'{who}: the gradient of {name(*args)} is sparse; sparse gradients are not built')
  if g.dtype != torch.float32:
    raise TypeError(f'{who}: the gradient of {name(*args)} is {str(g.dtype).replace("torch.", "")}, not float32')


def _one_device(tensors, dev, who, what, name):
  """... and about where tensors are: on a HIP device, all on the one of the tensors before them (dev, None in front of the first) -> that
  device; name(i) names tensors[i]."""
  for i, t in enumerate(tensors):
    if _lib._REQUIRE_DEVICE and not t.is_cuda:
      raise RuntimeError(f'{who} needs {what} on a HIP device (cuda:N), there is no CPU fallback; {name(i)} is on {t.device}')
    if dev is None:
      dev = t.device
    elif t.device != dev:
      raise RuntimeError(f'{who}: {what} on more than one device: {name(i)} is on {t.device}, others on {dev} (one HIP device)')
  return dev


def _check_max_norm(value, who, what):
  if isinstance(value, torch.Tensor):
    raise ValueError(f'{who}: {what} must be a number, a tensor {what} is not built')
  value = float(value)
  if not (math.isfinite(value) and value > 0.0):
    raise ValueError(f'{who}: {what} must be a finite number above 0, got {value}')
  return value


def _written(tensors):
  """A kernel wrote these tensors through their raw pointers: advance their version counters, as an in-place torch op would have, so that
  whatever is cached by (data_ptr, _version) -- the packed inference weights -- is rebuilt.  No launch."""
  if not tensors:
    return
  if _increment_version is None:
    for t in tensors:
      t.add_(0)
    return
  try:
    _increment_version(tensors)
  except TypeError:  # (a torch whose helper takes one tensor)
    for t in tensors:
      _increment_version(t)


def _name(gi, pi, p):
  return f'parameter {pi} of group {gi} {tuple(p.shape)}'


class AdamX(torch.optim.Optimizer):
  """``torch.optim.Adam(params, lr, betas, eps, weight_decay, amsgrad, maximize=, capturable=, decoupled_weight_decay=)``, the whole constructor, with
  the whole update in one HIP launch (module docstring).  ``extended_kernel = True`` sends every step through ``dyn_adamx_step`` even when no
  group asks for one of its options (A/B tests and tools/optimbench.py)."""

  extended_kernel = False

  def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
               capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
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
    if not 0.0 <= weight_decay:
      raise ValueError(f'Invalid weight_decay value: {weight_decay}')
    if foreach is not None or fused is not None:
      raise NotImplementedError('dynibar_amd.optim.Adam: foreach / fused choose among torch\'s implementations; this optimizer has one kernel')
    defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                    capturable=capturable, differentiable=differentiable, fused=None)
    if _TORCH_HAS_DECOUPLED or decoupled_weight_decay:
      defaults['decoupled_weight_decay'] = bool(decoupled_weight_decay)
    self._tables = None     # what depends on the parameter set alone (_new_tables), the staging buffers of its records included
    self._cleared = {}      # id(parameter) -> (gradient tensor, its version) as the last step(zero_grads=True) left it
    self._grad_stats = None  # the views into the tables' DynGradStats, once a guarded step has written them
    super().__init__(params, defaults)

  # ---- torch's layout of groups and state ------------------------------------------------------------------------------------------
  @staticmethod
  def _check_group(group, gi):
    for opt in _UNBUILT:
      if group.get(opt, False):
        raise NotImplementedError(f'dynibar_amd.optim.Adam: {opt}=True (group {gi}) is not built')
    wd = group.get('weight_decay', 0)
    if isinstance(wd, torch.Tensor) or not 0.0 <= wd:
      raise ValueError(f'dynibar_amd.optim.Adam: weight_decay of group {gi} must be a number >= 0, got {wd!r}')
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
          st['step'] = torch.tensor(float(st['step']), dtype=torch.float32, device=p.device if group['capturable'] else 'cpu')

  def load_state_dict(self, state_dict):
    """torch's, then the device-resident step counts of capturable groups: torch's loader casts every state tensor except ``step`` to the
    parameter's dtype, so ``beta_pow`` (float64 ``[beta1^t, beta2^t]``) is taken from the checkpoint itself, bit for bit.  A checkpoint without
    it -- one that ``torch.optim.Adam`` / ``AdamW`` saved -- gets ``[beta1 ** t, beta2 ** t]`` formed here on the host in double from the
    checkpoint's ``step`` and uploaded once (reading a device ``step`` is the one synchronisation of a load).  Groups that are not capturable
    carry no ``beta_pow``."""
    super().load_state_dict(state_dict)
    saved_ids = [i for g in state_dict['param_groups'] for i in g['params']]
    mine = [(g, p) for g in self.param_groups for p in g['params']]
    for pid, (group, p) in zip(saved_ids, mine):
      st = self.state.get(p)
      if not st:
        continue
      if not group['capturable']:
        st.pop('beta_pow', None)
        continue
      saved = state_dict['state'].get(pid, {}).get('beta_pow')
      if torch.is_tensor(saved) and saved.dtype == torch.float64 and saved.numel() == 2:
        st['beta_pow'] = saved.detach().reshape(2).to(p.device, copy=True)
      else:
        st.pop('beta_pow', None)
        self._device_counts(st, p, group)

  @staticmethod
  def _device_counts(st, p, group):
    """capturable: ``step`` a float32 0-d tensor and ``beta_pow`` float64 [2] on the parameter's device (made from the host's count where missing)"""
    step, pw = st['step'], st.get('beta_pow')
    if not (torch.is_tensor(pw) and pw.dtype == torch.float64 and pw.shape == (2,) and pw.device == p.device and pw.is_contiguous()):
      t = float(step)
      beta1, beta2 = group['betas']
      st['beta_pow'] = torch.tensor([beta1 ** t, beta2 ** t], dtype=torch.float64).to(p.device)
    if step.device != p.device or step.dtype != torch.float32 or step.dim() != 0:
      st['step'] = step.detach().to(device=p.device, dtype=torch.float32).reshape(())

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
    """Every check that can refuse, before anything is changed or launched -> (device, [(group index, parameter, gradient or None,
    the state of a parameter with a gradient or None before its first step)])."""
    entries = []
    for gi, group in enumerate(self.param_groups):
      self._check_group(group, gi)
      moments = ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq') if group.get('amsgrad', False) else ('exp_avg', 'exp_avg_sq')
      for pi, p in enumerate(group['params']):
        if p.dtype != torch.float32:
          raise TypeError(f'dynibar_amd.optim.Adam: {_name(gi, pi, p)} is {str(p.dtype).replace("torch.", "")}; the kernel updates float32 only')
        if p.is_sparse or p.layout != torch.strided:
          raise RuntimeError(f'dynibar_amd.optim.Adam: {_name(gi, pi, p)} is not a dense tensor')
        if not p.is_contiguous():
          raise ValueError(f'dynibar_amd.optim.Adam: {_name(gi, pi, p)} is not contiguous')
        if p.numel() >= 2 ** 31:
          raise ValueError(f'dynibar_amd.optim.Adam: {_name(gi, pi, p)} has {p.numel()} elements (below 2^31 per tensor)')
        g, st = p.grad, None
        if g is not None:
          _check_gradient(g, 'dynibar_amd.optim.Adam', _name, gi, pi, p)
          if g.shape != p.shape or g.device != p.device:
            raise ValueError(f'dynibar_amd.optim.Adam: the gradient of {_name(gi, pi, p)} is {tuple(g.shape)} on {g.device}, '
                             f'its parameter is on {p.device}')
          st = self.state.get(p)
          if st:
            for key in moments:
              m = st[key] if key != 'max_exp_avg_sq' else st.get(key, st['exp_avg_sq'])  # (made by the step where a checkpoint lacks it)
              if m.dtype != torch.float32 or m.shape != p.shape or m.device != p.device or not m.is_contiguous():
                raise ValueError(f'dynibar_amd.optim.Adam: {key} of {_name(gi, pi, p)} must be contiguous float32 {tuple(p.shape)} on {p.device}, '
                                 f'got {str(m.dtype).replace("torch.", "")} {tuple(m.shape)} on {m.device}')
        entries.append((gi, p, g, st))

    def name(i):  # (the entries are in the groups' order)
      gi, p = entries[i][:2]
      return _name(gi, i - sum(len(group['params']) for group in self.param_groups[:gi]), p)
    # where the tensors are, after what they are
    return _one_device([e[1] for e in entries], None, 'dynibar_amd.optim.Adam', 'parameters', name), entries

  @property
  def _staging(self):
    return self._tables['staging'] if self._tables else []

  @property
  def grad_stats(self):
    """``GradStats`` of the last guarded step (device tensor views; reading one synchronises), None before the first."""
    return self.__dict__.get('_grad_stats')

  def _tables_for(self, dev, sizes):
    """The tables of this parameter set on this device, made anew when one of the two changes or the step changes kernels."""
    # the plain kernels unless a group asks for what only the extended step has: defaults change nothing
    extended = bool(self.extended_kernel) or any(g.get('weight_decay', 0) != 0 or any(g.get(o, False) for o in _EXTENDED) for g in self.param_groups)
    tab = self._tables
    if tab is None or tab['device'] != dev or tab['sizes'] != sizes or tab['extended'] != extended:
      self._grad_stats = None
      tab = self._tables = _new_tables(dev, sizes, extended)
    return tab

  def _group_constants(self):
    """What a group's options come to, once per step and not once per tensor -> ([(group, lr, beta1, beta2, capturable, amsgrad)],
    float64 [groups, 10]: c1, c2, beta2, eps; wd, decay, flags; lr, beta1, beta2 for the device's scalars)"""
    per_group, consts = [], []
    for group in self.param_groups:
      lr, (beta1, beta2), lam = group['lr'], group['betas'], group.get('weight_decay', 0)
      decoupled = lam != 0 and bool(group.get('decoupled_weight_decay', False))
      per_group.append((group, lr, beta1, beta2, bool(group.get('capturable', False)), bool(group.get('amsgrad', False))))
      # (the decoupled factor in double here, fp32 in the record: rounded once)
      consts.append((1 - beta1, 1 - beta2, beta2, group['eps'], 0.0 if decoupled else lam, 1 - lr * lam if decoupled else 1.0,
                     1 if group.get('maximize', False) else 0, lr, beta1, beta2))
    return per_group, np.array(consts, np.float64)

  @staticmethod
  def _first_state(st, p, capturable):
    """torch's layout of a first-seen parameter's state (max_exp_avg_sq and beta_pow are made where a step first needs them)"""
    st['step'] = torch.zeros((), dtype=torch.float32, device=p.device) if capturable else torch.tensor(0.0, dtype=torch.float32)
    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)

  def _columns(self, entries, sizes, per_group, extended, zero_grads):
    """Every tensor that steps: its state, its count advanced where the host keeps it, the pointers and scalars of its record -> the records'
    columns (ptr, a, s2, skip, advance) and what the bookkeeping after the launch needs (copies, cleared, stepped)"""
    n = len(entries)
    ptr = {k: [0] * n for k in (('p', 'g', 'm', 'v', 'vmax', 'pow', 'step') if extended else 'pgmv')}
    a, s2, skip = [0.0] * n, [0.0] * n, [1] * n
    scalars, copies, cleared, stepped, advance = {}, [], {}, [], 0
    for i, (gi, p, g, st) in enumerate(entries):
      if g is None or sizes[i] == 0:
        continue
      group, lr, beta1, beta2, capturable, amsgrad = per_group[gi]
      if not st:
        st = self.state[p]
        self._first_state(st, p, capturable)
      if capturable:  # the count lives on the device: k_adam_advance is its only writer, a held step leaves it alone
        self._device_counts(st, p, group)
        ptr['pow'][i], ptr['step'][i] = st['beta_pow'].data_ptr(), st['step'].data_ptr()
        advance = 1
      else:
        step = st['step']
        if step.is_cuda:  # (a group switched back from capturable: one synchronisation)
          step = st['step'] = step.detach().cpu()
        step += 1
        key = (lr, beta1, beta2, step.item())
        if key not in scalars:
          scalars[key] = step_scalars(*key)
        a[i], s2[i] = scalars[key]
      if amsgrad:
        if 'max_exp_avg_sq' not in st:
          st['max_exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        ptr['vmax'][i] = st['max_exp_avg_sq'].data_ptr()
      gc = g if g.is_contiguous() else _contiguous(g, copies)  # (a copy lives until the launch is enqueued)
      ptr['p'][i], ptr['g'][i], ptr['m'][i], ptr['v'][i] = p.data_ptr(), gc.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr()
      skip[i] = 0
      stepped.append(p)
      if zero_grads:
        cleared[id(p)] = g
    return types.SimpleNamespace(ptr=ptr, a=a, s2=s2, skip=skip, advance=advance, copies=copies, cleared=cleared, stepped=stepped)

  @staticmethod
  def _fill(host, entries, sizes, w, consts, extended):
    """The records of this step into a staging buffer: DynAdamTensor rows and, for the extended step, the DynAdamXTensor rows behind them."""
    n = len(entries)
    rec = _records(host, {k: w.ptr[k] for k in 'pgmv'}, sizes, w.skip)
    const = consts[[e[0] for e in entries]]  # [n, 10]: each tensor's group constants
    rec['a'], rec['s2'] = w.a, w.s2
    rec['c1'], rec['c2'], rec['beta2'], rec['eps'] = const[:, 0], const[:, 1], const[:, 2], const[:, 3]
    if extended:
      xrec = host.numpy()[n * RECORD.itemsize:n * (RECORD.itemsize + XRECORD.itemsize)].view(XRECORD)
      for k in RECORD.names[:-1]:
        xrec[k] = rec[k]
      for k in ('vmax', 'pow', 'step'):
        xrec[k] = w.ptr[k]
      xrec['wd'], xrec['decay'], xrec['flags'], xrec['lr_d'], xrec['beta1_d'], xrec['beta2_d'] = (const[:, j] for j in range(4, 10))

  def _launch(self, tab, table, like, advance, zero_grads, guarded, max_grad_norm, skip_nonfinite):
    """dyn_grad_norm in front of a guarded step, then the one entry point of (extended, guarded)."""
    stream, extended = stream_of(like), tab['extended']
    fields = dict(table, zero_grads=1 if zero_grads else 0)
    if extended:  # its records lie behind the plain ones, which the norm reads
      fields.update(tensors=ctypes.c_void_p(table['tensors'].value + table['n_tensors'] * RECORD.itemsize), advance=advance)
    if guarded:
      stats = ctypes.c_void_p(tab['stats'].data_ptr())
      call('dyn_grad_norm', params('DynGradNormParams', partials=ctypes.c_void_p(tab['partials'].data_ptr()), stats=stats,
                                   max_norm=0.0 if max_grad_norm is None else max_grad_norm, count=1, **table), stream)
      fields.update(skip_nonfinite=1 if skip_nonfinite else 0, stats=stats)
    entry, struct = _STEP_CALLS[extended, guarded]
    call(entry, params(struct, **fields), stream)
    if guarded:
      self._grad_stats = tab['grad_stats']

  def _after(self, w, zero_grads):
    """The kernel wrote the parameters through raw pointers, and with zero_grads the gradients it read."""
    _written(w.stepped)
    if zero_grads:
      for g, _ in w.copies:  # the kernel cleared the contiguous copy, not the strided gradient itself
        g.zero_()
      self._cleared = {k: (g, g._version) for k, g in w.cleared.items()}

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
    if dev is None or all(e[2] is None for e in entries):
      return loss
    sizes = [e[1].numel() for e in entries]
    tab = self._tables_for(dev, sizes)
    if tab['n_chunks'] == 0:
      return loss
    per_group, consts = self._group_constants()
    w = self._columns(entries, sizes, per_group, tab['extended'], zero_grads)
    host, event = _stage_in(tab)
    self._fill(host, entries, sizes, w, consts, tab['extended'])
    self._launch(tab, _send(tab, host, event), entries[0][1], w.advance, zero_grads, guarded, max_grad_norm, skip_nonfinite)
    self._after(w, zero_grads)
    return loss


class Adam(AdamX):
  """``torch.optim.Adam(params, lr, betas, eps)`` with the whole update in one HIP launch: the optimizer of the reference's training loop, as it
  was before ``AdamX``.  It keeps refusing ``amsgrad``, ``maximize``, ``capturable`` and ``weight_decay != 0`` by name -- a script that sets one of
  them changes its class to ``AdamX`` (or ``AdamW``) in the same line -- and always launches the plain kernels."""

  def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
               capturable=False, differentiable=False, fused=None):
    super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                     differentiable=differentiable, fused=fused)

  @staticmethod
  def _check_group(group, gi):
    for opt in _EXTENDED + _UNBUILT:
      if group.get(opt, False):
        raise NotImplementedError(f'dynibar_amd.optim.Adam: {opt}=True (group {gi}) is not built' +
                                  (' in this class; dynibar_amd.optim.AdamX has it' if opt in _EXTENDED else ''))
    if group.get('weight_decay', 0) != 0:
      raise NotImplementedError(f'dynibar_amd.optim.Adam: weight_decay={group["weight_decay"]} (group {gi}) is not built in this class; '
                                'dynibar_amd.optim.AdamX (coupled) and AdamW (decoupled) have it')
    AdamX._check_group(group, gi)


class AdamW(AdamX):
  """``torch.optim.AdamW``: ``AdamX`` with ``decoupled_weight_decay=True`` and torch's default ``weight_decay=1e-2`` -- the parameter is multiplied by
  ``fp32(1 - lr * weight_decay)`` and the moments never see the decay.  Its ``state_dict`` loads into ``torch.optim.AdamW`` and back."""

  def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
               capturable=False, differentiable=False, fused=None):
    super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                     differentiable=differentiable, fused=fused, decoupled_weight_decay=True)

  def __setstate__(self, state):
    super().__setstate__(state)
    for group in self.param_groups:
      group['decoupled_weight_decay'] = True  # (torch.optim.AdamW.__setstate__ does the same: a group of an AdamW is always decoupled)


# ---- the norm and the clip on their own ----------------------------------------------------------------------------------------------
_TABLES = collections.OrderedDict()  # (device, sizes) -> tables, for grad_norm / clip_grad_norm_
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
    _check_gradient(g, who, lambda: f'parameter {i} {tuple(p.shape)}')
    if g.numel() >= 2 ** 31:
      raise ValueError(f'{who}: the gradient of parameter {i} has {g.numel()} elements (below 2^31 per tensor)')
    dev = _one_device((g,), dev, who, 'gradients', lambda _: f'that of parameter {i}')
    grads.append(g)
  return dev, grads


def _norm_of(grads, dev, max_norm):
  """dyn_grad_norm over the gradients -> (tables, the call's table fields, [(strided gradient, its contiguous copy)])"""
  sizes = [g.numel() for g in grads]
  key = (str(dev), tuple(sizes))
  tab = _TABLES.get(key)
  if tab is None:
    tab = _TABLES[key] = _new_tables(dev, sizes)
    while len(_TABLES) > _TABLES_KEPT:
      _TABLES.popitem(last=False)
  else:
    _TABLES.move_to_end(key)
  copies = []
  host, event = _stage_in(tab)
  _records(host, {'g': [(g if g.is_contiguous() else _contiguous(g, copies)).data_ptr() for g in grads]}, sizes, [1 if n == 0 else 0 for n in sizes])
  table = _send(tab, host, event)
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
