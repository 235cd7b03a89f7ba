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

Not built, refused by name: amsgrad, maximize, weight_decay, capturable, differentiable, an explicit foreach / fused.  Tensors must be
contiguous fp32 on ONE HIP device: there is no CPU fallback, host tensors are refused.
"""
from __future__ import annotations

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

_NP_OF = {ctypes.c_void_p: '<u8', ctypes.c_int64: '<i8', ctypes.c_float: '<f4', ctypes.c_int32: '<i4'}
RECORD = np.dtype([(name, _NP_OF[ct]) for name, ct in _lib._STRUCT_SPECS['DynAdamTensor']])
assert RECORD.itemsize == ctypes.sizeof(_lib.STRUCTS['DynAdamTensor']) and RECORD.itemsize % 8 == 0

_UNBUILT = ('amsgrad', 'maximize', 'capturable', 'differentiable')
_TORCH_HAS_DECOUPLED = 'decoupled_weight_decay' in inspect.signature(torch.optim.Adam.__init__).parameters


def step_scalars(lr, beta1, beta2, t):
  """(a, s2) of the contract for a step count t >= 1: torch's own double arithmetic (``1 - beta ** step``, ``lr / bias_correction1``,
  ``bias_correction2 ** 0.5``), each result rounded to fp32 once."""
  bias_correction1 = 1 - beta1 ** t
  bias_correction2 = 1 - beta2 ** t
  return np.float32(-(lr / bias_correction1)), np.float32(math.sqrt(bias_correction2))


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

  def __setstate__(self, state):
    super().__setstate__(state)
    self.__dict__.setdefault('_staging', [])
    self.__dict__.setdefault('_cleared', {})
    self._tables = None
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
    """The chunk list of a parameter set (uploaded once) and the device buffer its records go to."""
    chunks = np.concatenate([np.stack([np.full(-(-n // CHUNK), i, np.int32), np.arange(-(-n // CHUNK), dtype=np.int32)], axis=1)
                             for i, n in enumerate(sizes)] or [np.zeros((0, 2), np.int32)])
    host = torch.from_numpy(np.ascontiguousarray(chunks))
    nbytes = max(1, len(sizes)) * RECORD.itemsize
    if dev.type == 'cuda':
      with torch.cuda.device(dev):
        chunks_dev = host.pin_memory().to(dev, non_blocking=True) if len(chunks) else host.to(dev)
        records_dev = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    else:  # (the emulator build of the tests: the "device" is the host)
      chunks_dev, records_dev = host, None
    self._staging = []
    self._tables = dict(device=dev, sizes=sizes, n_chunks=int(len(chunks)), chunks=chunks_dev, records=records_dev, nbytes=nbytes)

  def _stage(self, dev, nbytes):
    """A host buffer for this step's records that no earlier copy still reads: pinned, with the event of its last copy."""
    if dev.type != 'cuda':
      if not self._staging:
        self._staging.append((torch.empty((nbytes,), dtype=torch.uint8), None))
      return self._staging[0]
    for buf, ev in self._staging:
      if ev.query():
        return buf, ev
    entry = (torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
    self._staging.append(entry)
    return entry

  @torch.no_grad()
  def step(self, closure=None, zero_grads=False):
    """One ``k_adam_step`` launch over every parameter that has a gradient.  zero_grads: the launch also stores 0 to the gradients it read."""
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
    if dev.type == 'cuda':
      with torch.cuda.device(dev):
        tab['records'].copy_(host, non_blocking=True)
        event.record(torch.cuda.current_stream(dev))
      records = tab['records']
    else:
      records = host
    like = entries[0][1]
    call('dyn_adam_step', params('DynAdamParams', tensors=ctypes.c_void_p(records.data_ptr()), n_tensors=n,
                                 chunks=ctypes.c_void_p(tab['chunks'].data_ptr()), n_chunks=tab['n_chunks'], zero_grads=1 if zero_grads else 0),
         stream_of(like))
    if zero_grads:
      for g, _ in copies:  # the kernel cleared the contiguous copy, not the strided gradient itself
        g.zero_()
      self._cleared = {k: (g, g._version) for k, g in cleared.items()}
    return loss
