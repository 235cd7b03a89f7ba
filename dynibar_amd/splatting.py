"""Drop-in for the third-party ``splatting`` package's ``splatting_function`` (render_source_vv.py:12, :58), on the gfx950 kernels.

    from splatting import splatting_function   ->   from dynibar_amd.splatting import splatting_function

The four modes and their argument checks are the package's: ``summation`` (no metric), ``average`` (a ones channel appended),
``linear`` (``cat[frame * m, m]``) and ``softmax`` (the same with ``m = exp(metric)``, formed by torch as the package does); the
normalised modes return ``out[:, :-1] / (out[:, -1:] + eps)``.  The splat itself is one ``dyn_splat`` call (k_splat_keys, the radix
sort, k_splat_resolve): every output pixel is summed in ascending contribution id, so the result is bitwise reproducible
(include/dynibar_hip.h).  Forward only, fp32, device tensors only.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import call, params, ptr, stream_of

MODES = ('summation', 'average', 'linear', 'softmax')


def workspace(B, H, W, device):
  need = int(_lib.lib().dyn_splat_workspace_bytes(B, H, W))
  if need == 0:
    raise ValueError(f'splat of B={B} H={H} W={W} is unsupported (B*H*W must not exceed 2^28)')
  return torch.empty((need,), dtype=torch.uint8, device=device), need


def _no_grad_inputs(*ts):
  if torch.is_grad_enabled() and any(getattr(t, 'requires_grad', False) for t in ts):
    raise RuntimeError('dynibar_amd.splatting is forward only: call it under torch.no_grad() or on detached tensors '
                       '(the reference detaches its inputs, render_source_vv.py:58-60)')


def splat(frame, flow, multiplier=None, normalize=False, eps=1e-7):
  """The summation splat of ``frame`` [B,C,H,W] along ``flow`` [B,2,H,W]; with ``multiplier`` [B,H,W] every contribution is
  w * (frame * multiplier); ``normalize``: out = num / (den + eps), den the splatted multiplier (or weight).  One dyn_splat call."""
  B, C, H, W = frame.shape
  out = torch.empty((B, C, H, W), dtype=torch.float32, device=frame.device)
  ws, need = workspace(B, H, W, frame.device)
  fr, fl = frame.contiguous(), flow.contiguous()
  mu = None if multiplier is None else multiplier.contiguous()
  p = params('DynSplatParams', B=B, C=C, H=H, W=W, frame=ptr(fr), flow=ptr(fl), multiplier=ptr(mu), normalize=1 if normalize else 0,
             eps=float(eps), out=ptr(out), workspace=ptr(ws, torch.uint8), workspace_bytes=need)
  call('dyn_splat', p, stream_of(fr))
  return out


def splatting_function(splatting_type, frame, flow, importance_metric=None, eps=1e-7):
  """splatting.splatting_function(splatting_type, frame, flow, importance_metric=None, eps=1e-7) on the HIP kernels."""
  if splatting_type == 'summation':
    assert importance_metric is None
  elif splatting_type == 'average':
    assert importance_metric is None
  elif splatting_type in ('linear', 'softmax'):
    assert isinstance(importance_metric, torch.Tensor)
    assert importance_metric.shape == (frame.shape[0], 1, frame.shape[2], frame.shape[3])
  else:
    raise NotImplementedError('splatting_type has to be one of {summation, average, linear, softmax}')
  assert frame.dtype == flow.dtype
  assert frame.device == flow.device
  assert len(frame.shape) == 4
  assert len(flow.shape) == 4
  assert frame.shape[0] == flow.shape[0]
  assert frame.shape[2] == flow.shape[2]
  assert frame.shape[3] == flow.shape[3]
  assert flow.shape[1] == 2
  _no_grad_inputs(frame, flow, importance_metric)
  if frame.dtype != torch.float32:
    raise TypeError(f'dynibar_amd.splatting computes in fp32; got {frame.dtype}')
  with torch.no_grad():
    m = None
    if splatting_type == 'linear':
      m = importance_metric.float()[:, 0]
    elif splatting_type == 'softmax':
      m = importance_metric.float().exp()[:, 0]
    return splat(frame, flow, m, normalize=splatting_type != 'summation', eps=eps)
