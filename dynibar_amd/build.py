"""Build libdynibar_hip.so (and its two engine flavours, _x6 and _x1) for gfx950 in-tree (dynibar_amd/csrc/).   python -m dynibar_amd.build [--force]

Translation units: the geometry/compositing kernels are compiled with -ffp-contract=off (bit-exact sample depths,
points and indices versus the reference's un-fused fp32 ops), the MFMA network kernels and the feature encoder with default contraction.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OUT = os.path.join(CSRC, 'libdynibar_hip.so')
OUT_X6 = os.path.join(CSRC, 'libdynibar_hip_x6.so')
OUT_X1 = os.path.join(CSRC, 'libdynibar_hip_x1.so')
UNITS = [
    ('dyn_geometry.hip', ['-ffp-contract=off', '-munsafe-fp-atomics']),
    ('dyn_nets.hip', []),
    ('dyn_encoder.hip', ['-munsafe-fp-atomics']),  # (the training form's col2im adds with hardware fp32 atomics, not CAS loops)
    ('dyn_train.hip', ['-munsafe-fp-atomics']),
    ('dyn_comm.hip', []),  # the RCCL pixel gather (RCCL itself is resolved at run time: no link dependency)
]
COMMON = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function']
# The other flavours of the network unit (dynibar_amd.engine), each linked with the same other units into a library of its own:
FLAVOURS = [
    # the fp32-class 6-term split engine: used by the precision A/B test and bench leg
    ('dyn_nets_x6.o', OUT_X6, ['-DDYN_SPLIT_TERMS=6', '-DDYN_SPLIT_F16=0']),
    # the one-product half-float engine: the `half` engine, for preview rendering
    ('dyn_nets_x1.o', OUT_X1, ['-DDYN_SPLIT_TERMS=1']),
]


def _deps():
  return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(('.hip', '.h'))] + [
      os.path.join(os.path.dirname(HERE), 'include', 'dynibar_hip.h')]


STAMP = os.path.join(CSRC, '.build_stamp')


def _stamp():
  """sha256 over the sources, headers and flags (every flavour's, and this recipe itself) the libraries are made from.  (Modification times are not
  enough: a build that was started before an edit finishes after it and leaves a stale library that is newer than its sources.)"""
  import hashlib
  h = hashlib.sha256(repr((COMMON, UNITS, [(o, os.path.basename(out), f) for o, out, f in FLAVOURS])).encode())
  for d in sorted(_deps() + [os.path.abspath(__file__)]):
    h.update(os.path.basename(d).encode())
    with open(d, 'rb') as f:
      h.update(f.read())
  return h.hexdigest()


def build(force=False, verbose=True):
  hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
  units = [(s, f) for s, f in UNITS if os.path.exists(os.path.join(CSRC, s))]
  stamp = _stamp()
  if not force and all(os.path.exists(p) for p in [OUT, STAMP] + [out for _, out, _ in FLAVOURS]) and open(STAMP).read().strip() == stamp:
    return OUT
  if os.path.exists(STAMP):
    os.remove(STAMP)
  # the translation units are independent: compile them (and the 6-term and the one-product flavour of the network unit) side by side
  from concurrent.futures import ThreadPoolExecutor
  jobs = []
  for src, flags in units:
    obj = os.path.join(CSRC, src.replace('.hip', '.o'))
    jobs.append((obj, [hipcc] + COMMON + flags + ['-c', os.path.join(CSRC, src), '-o', obj]))
  for obj, _, flags in FLAVOURS:
    jobs.append((os.path.join(CSRC, obj), [hipcc] + COMMON + flags + ['-c', os.path.join(CSRC, 'dyn_nets.hip'), '-o', os.path.join(CSRC, obj)]))

  def run(job):
    if verbose:
      print(' '.join(job[1]), flush=True)
    subprocess.check_call(job[1])
    return job[0]

  with ThreadPoolExecutor(max_workers=int(os.environ.get('DYNIBAR_BUILD_JOBS', '6'))) as ex:
    built = list(ex.map(run, jobs))
  objs = built[:len(units)]
  cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC'] + objs + ['-ldl', '-o', OUT]
  if verbose:
    print(' '.join(cmd), flush=True)
  subprocess.check_call(cmd)
  for flavour, (_, out, _) in zip(built[len(units):], FLAVOURS):  # the same units with another flavour of the network unit
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', objs[0], flavour] + objs[2:] + ['-ldl', '-o', out])
  if _stamp() == stamp:  # the sources did not change while the compilers ran
    with open(STAMP, 'w') as f:
      f.write(stamp + '\n')
  return OUT


if __name__ == '__main__':
  print(build(force='--force' in sys.argv))
