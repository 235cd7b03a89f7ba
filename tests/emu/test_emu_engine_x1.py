"""The one-product half-float engine build (csrc/dyn_mlp.h, DYN_SPLIT_TERMS == 1: libdynibar_hip_x1.so) under the wave-level emulator: the network unit
compiled with -DDYN_SPLIT_TERMS=1 beside the default objects of tests/emu/_build, checked by tests/engine_x1_checks.py.  Catches fragment-map, packing and
rounding mistakes in a container without a GPU; tests/test_gpu_engine_x1.py is authoritative."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import engine_x1_checks as X

pytestmark = pytest.mark.emu


@pytest.fixture(scope='module')
def emu_x1():
  """libdynibar_emu_x1.so: dyn_nets.hip with one half per operand, every other object shared with the default emulator library"""
  import emu_build
  from dynibar_amd import _lib
  emu_build.build()  # the default library: its objects are reused
  src = os.path.join(emu_build.CSRC, 'dyn_nets.hip')
  obj = os.path.join(emu_build.OUT_DIR, 'dyn_nets_x1.o')
  out = os.path.join(emu_build.OUT_DIR, 'libdynibar_emu_x1.so')
  deps = [os.path.join(emu_build.CSRC, f) for f in os.listdir(emu_build.CSRC) if f.endswith('.h')] + [
      src, os.path.join(emu_build.HERE, 'hip', 'hip_runtime.h'), os.path.join(emu_build.ROOT, 'include', 'dynibar_hip.h')]
  common = [emu_build.CXX, '-std=c++20', '-O2', '-g', '-pthread', '-fPIC', '-I', emu_build.HERE, '-Wno-unused-function']
  if not (os.path.exists(obj) and all(os.path.getmtime(obj) >= os.path.getmtime(d) for d in deps)):
    subprocess.check_call(common + ['-DDYN_SPLIT_TERMS=1', '-x', 'c++', '-c', src, '-o', obj])
  others = [os.path.join(emu_build.OUT_DIR, s.replace('.hip', '.o')) for s, _ in emu_build.UNITS if s != 'dyn_nets.hip' and os.path.exists(os.path.join(emu_build.CSRC, s))]
  subprocess.check_call(common + ['-shared', obj] + others + [os.path.join(emu_build.OUT_DIR, 'emu_runtime.o'), '-o', out])
  _lib._install_for_tests(ctypes.CDLL(out), require_device=False)
  yield 'cpu'
  _lib._install_for_tests(None, require_device=True)


def test_library_describes_itself(emu_x1):
  from dynibar_amd import _lib
  assert _lib.lib().dyn_mlp_split_terms() == 1 and _lib.lib().dyn_mlp_split_kind() == 2


def test_engine_rounds_to_nearest(emu_x1):
  """float64 on half-rounded operands at 3e-6 + the midpoint term: a truncating convert or a mis-packed weight image is far outside"""
  X.check_selftest(emu_x1, rows=70)


def test_engine_range_edges(emu_x1):
  X.check_selftest_ranges(emu_x1, rows=70)


@pytest.mark.parametrize('case', sorted(X.EMU_CASES))
def test_networks_against_the_half_rounded_oracle(emu_x1, case):
  X.EMU_CASES[case](emu_x1)
