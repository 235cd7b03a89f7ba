"""tools/enginebench.py off the GPU: it starts, its chain sums are keyed on profile slots the library really has, and a chain that matches no kernel
is an error instead of an empty sum."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'enginebench.py')


@pytest.fixture(scope='module')
def tool():
  spec = importlib.util.spec_from_file_location('enginebench_under_test', TOOL)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def profile_slots():
  """the names dyn_profile_name returns, from the table in dyn_geometry.hip"""
  src = open(os.path.join(ROOT, 'dynibar_amd', 'csrc', 'dyn_geometry.hip')).read()
  table = re.search(r'g_prof_names\[\w*\]\s*=\s*\{(.*?)\}', src, flags=re.S).group(1)
  return re.findall(r'"(k_\w+)"', table)


def test_help_runs_without_a_gpu():
  r = subprocess.run([sys.executable, TOOL, '--help'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0 and '--exact' in r.stdout and '--out' in r.stdout, r.stderr


def test_chains_name_real_profile_slots(tool):
  slots = profile_slots()
  assert 'k_static_points' in slots and len(slots) > 20
  tool.check_chains(slots)  # raises SystemExit on a name the library does not have
  assert {'k_static_views', 'k_dynamic_views'} <= set(tool.CHAINS['view chain'])
  assert {'k_static_points', 'k_dynamic_points'} <= set(tool.CHAINS['point chain']) and 'k_motion_mlp' not in tool.CHAINS['point chain']
  assert tool.CHAINS['motion MLP'] == ('k_motion_mlp',) and 'motion MLP' not in tool.chains_of('step') and 'motion MLP' in tool.chains_of('frame')
  with pytest.raises(SystemExit, match='k_net_points'):
    _stale(tool, slots)


def _stale(tool, slots):
  old = dict(tool.CHAINS)
  tool.CHAINS['point chain'] = ('k_net_points',)
  try:
    tool.check_chains(slots)
  finally:
    tool.CHAINS.clear()
    tool.CHAINS.update(old)


def test_the_workloads_the_children_run_exist():
  """the child builds bench.StaticStep(dev, R, S, V), tools/frame_case.FrameCase(dev, H, W, vdy, vst, chunk) and sets render_image.CHUNK_STREAMS"""
  import inspect
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import bench
    import frame_case
    from dynibar_amd import render_image
  finally:
    sys.path.remove(os.path.join(ROOT, 'tools'))
  assert list(inspect.signature(bench.StaticStep.__init__).parameters)[1:5] == ['dev', 'R', 'S', 'V'] and hasattr(bench.StaticStep, 'step')
  assert list(inspect.signature(frame_case.FrameCase.__init__).parameters)[1:7] == ['dev', 'H', 'W', 'vdy', 'vst', 'chunk']
  assert hasattr(frame_case.FrameCase, 'sampler') and hasattr(frame_case.FrameCase, 'render')
  assert isinstance(render_image.CHUNK_STREAMS, int)
  src = inspect.getsource(render_image)
  assert len(re.findall(r'\bCHUNK_STREAMS\b', src)) >= 2 and not re.search(r'def \w+\([^)]*=\s*CHUNK_STREAMS', src), 'CHUNK_STREAMS must be read at call time'


def test_report_sums_every_chain_and_refuses_an_empty_one(tool):
  eng = lambda n, t: dict(name=n, terms=t, kind=2, path=f'/x/lib_{n}.so')
  k = lambda s: {n: dict(ms=ms * s, launches=1) for n, ms in (('k_static_views', 2.0), ('k_static_points', 0.5), ('k_motion_mlp', 0.25), ('k_static_blend', 0.125))}
  res = {n: dict(engine=eng(n, t), step_ms=[1.0 * s] * 3, frame_ms=[10.0 * s] * 2, chunk_streams=2, step_kernels=k(s), frame_kernels=k(s))
         for n, t, s in (('split', 3, 1.0), ('half', 1, 0.5))}
  txt = tool.report(res, {})
  row = [l for l in txt.splitlines() if l.strip().startswith('point chain (sum)')][0]
  assert '0.500' in row and '0.250' in row and row.rstrip().endswith('0.500'), row  # the point kernels, without k_motion_mlp
  assert len([l for l in txt.splitlines() if l.strip().startswith('motion MLP (sum)')]) == 1  # (the frame's table only)
  res['half']['step_kernels'] = {n: v for n, v in k(0.5).items() if n != 'k_static_blend'}
  with pytest.raises(SystemExit, match='k_static_blend'):
    tool.report(res, {})
