"""Which flavour of the network engine this process runs.

  'split' (default)  libdynibar_hip.so     two half-float parts per operand, three partial products: fp32-class products
  'exact'            libdynibar_hip_x6.so  three bf16 parts per operand, six partial products: all 24 bits
  'half'             libdynibar_hip_x1.so  one half per operand, one product: TF32-class operands (what the reference's A100 runs multiplied
                                           with), for preview rendering

The flavours differ in the inference network kernels only (dyn_nets.hip); the encoder, the geometry kernels and the training kernels are the same
code in all three, so rendering under grad mode does not depend on the choice.  A process binds ONE library: select() must run before the first kernel
call, and there is no fallback -- asking for a flavour whose library has not been built is an error.  DYNIBAR_ENGINE=split|exact|half in the
environment selects the flavour at import; an explicit DYNIBAR_HIP_LIB path wins over both: select() refuses to override it.
"""
from __future__ import annotations

import os

from . import _lib


def select(name):
  """Make `name` the library the first kernel call will bind.  RuntimeError if a library is bound already or DYNIBAR_HIP_LIB names another file,
  ValueError for an unknown name."""
  path = _lib.engine_path(name)
  if _lib._LIB is not None:
    raise RuntimeError(f'engine.select({name!r}): {_lib.bound_path()} is already loaded (a process binds one library: select the engine before the first kernel call)')
  explicit = os.environ.get('DYNIBAR_HIP_LIB')
  if explicit:
    if os.path.realpath(explicit) == os.path.realpath(path):
      return  # (the explicit path is this flavour's file already)
    raise RuntimeError(f'engine.select({name!r}): DYNIBAR_HIP_LIB={explicit} is set and wins over the engine name (unset it to select by name)')
  if not os.path.exists(path):
    raise RuntimeError(f'{path} is missing: build the gfx950 kernels with `python -m dynibar_amd.build` (there is no fallback to another engine)')
  _lib.LIB_PATH = path


def current():
  """{'name', 'terms', 'kind', 'path'} of the library this process runs, read from the library itself (loads it if nothing is bound yet)."""
  L = _lib.lib()
  terms, kind = int(L.dyn_mlp_split_terms()), int(L.dyn_mlp_split_kind())
  name = {(3, 2): 'split', (6, 1): 'exact', (1, 2): 'half'}.get((terms, kind), f'custom ({terms} terms, kind {kind})')
  return dict(name=name, terms=terms, kind=kind, path=_lib.bound_path())
