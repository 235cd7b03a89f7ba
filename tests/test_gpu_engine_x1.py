"""-m gpu: the one-product half-float engine build (libdynibar_hip_x1.so, dynibar_amd.engine 'half').  A process binds one library, so every test starts one
child process with the x1 library selected and a time limit, and asserts on its exit status and on what it printed (tests/engine_x1_checks.py holds the
checks; the tables it prints are the record quoted in DESIGN.md section 5).  A missing library is a failure, not a skip."""
import os
import re
import subprocess
import sys

import pytest

import engine_x1_checks as X
from dynibar_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dynibar_amd', 'csrc')
LIB_X1 = os.path.join(CSRC, 'libdynibar_hip_x1.so')
CHECKS = os.path.join(ROOT, 'tests', 'engine_x1_checks.py')


def child(*argv, env=None, timeout=300):
  assert os.path.exists(LIB_X1), 'python -m dynibar_amd.build builds the three engine flavours: libdynibar_hip_x1.so is missing'
  e = {k: v for k, v in os.environ.items() if k not in ('DYNIBAR_HIP_LIB', 'DYNIBAR_ENGINE')}
  e['PYTHONPATH'] = os.pathsep.join([ROOT, os.path.join(ROOT, 'tests')] + ([e['PYTHONPATH']] if e.get('PYTHONPATH') else []))
  e.update(env if env is not None else {'DYNIBAR_HIP_LIB': LIB_X1})
  r = subprocess.run([sys.executable, CHECKS] + list(argv), env=e, capture_output=True, text=True, timeout=timeout)
  print(r.stdout)
  assert r.returncode == 0 and 'x1-check ok' in r.stdout, f'{" ".join(argv)}: exit status {r.returncode}\n{r.stdout}\n{r.stderr[-4000:]}'
  return r.stdout


def test_engine_selftest_rounding_and_ranges():
  """(a) float64 on half-rounded operands, 3e-6 + the midpoint term, 1000 rows; the tiny and huge activation ranges"""
  out = child('selftest')
  assert re.search(r'over the limit 0;', out) and 'activations 1e-06..6e-05' in out and 'activations 70000..120000' in out, out


@pytest.mark.parametrize('case', sorted(X.NETWORK_CASES))
def test_networks_against_the_half_rounded_oracle(case):
  """(b) per output, the kernels' error against float64 held to twice the half-rounded fp32 oracle's own"""
  assert 'x1 accuracy [' in child('network', case)


def test_render_rays_mv_against_the_reference():
  """(c) the coarse + fine path on the real reference's golden scene; two identical calls give identical bits"""
  assert 'max |rgb error| against the real reference' in child('path')


def test_frame_is_the_same_on_one_and_two_chunk_streams():
  assert 'bit-identical on one and on two chunk streams' in child('streams')


def test_environment_selects_the_engine():
  """(d) DYNIBAR_ENGINE=half binds the x1 library; a later engine.select raises and names it"""
  assert '"terms": 1' in child('interface_env', env={'DYNIBAR_ENGINE': 'half'})


def test_select_before_the_first_kernel_call():
  assert '"name": "half"' in child('interface_select', env={})


def test_explicit_library_path_wins_over_the_engine_name():
  assert '"terms": 3' in child('interface_lib_wins', env={'DYNIBAR_ENGINE': 'half', 'DYNIBAR_HIP_LIB': os.path.join(CSRC, 'libdynibar_hip.so')})


def test_unknown_engine_name_is_refused_at_import():
  e = dict(os.environ, DYNIBAR_ENGINE='fast', PYTHONPATH=ROOT)
  e.pop('DYNIBAR_HIP_LIB', None)
  r = subprocess.run([sys.executable, '-c', 'from dynibar_amd import _lib'], env=e, capture_output=True, text=True, timeout=120)
  assert r.returncode != 0 and 'ValueError' in r.stderr and "'fast'" in r.stderr, r.stderr


def test_x1_library_exports_the_header():
  """the three libraries export exactly what include/dynibar_hip.h declares"""
  declared = set(_lib._FUNC_SPECS)
  for name in _lib.ENGINE_LIBS.values():
    path = os.path.join(CSRC, name)
    assert os.path.exists(path), f'{name} is missing: python -m dynibar_amd.build builds the three engine flavours'
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith('dyn_') and l.split()[-2] in ('T', 'W')}
    assert exported == declared, f'{name}: only exported {sorted(exported - declared)}, only declared {sorted(declared - exported)}'
