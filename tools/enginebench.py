"""The engine flavours side by side (dynibar_amd.engine: split / half / exact) on the two workloads the project quotes: the bench step (BASELINE
configs[1]: 4096 rays x 64 samples x 8 views, static branch) and one 288 x 512 Nvidia-config frame (configs[2]: 64 + 64 samples, 7 dynamic + 11 static
views, chunk 8192) on synthetic data.  GPU only.

  python tools/enginebench.py [--exact] [--lib TAG=lib.so ...] [--steps 200] [--frames 2] [--out profiles/engine_x1_bench.txt]

--lib adds a developer build of the library as one more column (an A/B of kernel forms: e.g. the one-product unit compiled with -DDYN_POINTS_DUO=1).

A process binds one library, so every flavour runs in ONE fresh child process with DYNIBAR_HIP_LIB set; this parent never initialises the GPU.  One child
at a time, each under its own `timeout -k 10`; a child that fails ends the run (nothing more is started on the GPU).  Printed: ms per step and per frame,
the per-kernel averages of dyn_profile_* (taken on one chunk stream: overlapped kernels would be counted twice), the ratios half / split measured in
this same session, and the largest |rgb| difference of `half` (and `exact`) against `split` on the same rays.  No ratio is fixed in advance.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

# The chains by the names of the profile slots (dyn_profile_name: one slot per launch site, whichever kernel form the flavour takes there).
CHAINS = {'view chain': ('k_static_views', 'k_dynamic_views'),
          'point chain': ('k_static_points', 'k_dynamic_points', 'k_static_points_qkv', 'k_dynamic_points_qkv'),
          'motion MLP': ('k_motion_mlp',),
          'blend': ('k_static_blend',)}
NOT_IN_THE_STEP = ('motion MLP',)  # the bench step is the static branch alone


def chains_of(what):
  return {c: m for c, m in CHAINS.items() if what != 'step' or c not in NOT_IN_THE_STEP}


def _profile(lib, per):
  nk = lib.dyn_profile_count()
  ms, cnt = (ctypes.c_float * nk)(), (ctypes.c_int * nk)()
  lib.dyn_profile_read(ms, cnt)
  return {lib.dyn_profile_name(i).decode(): dict(ms=ms[i] / per, launches=cnt[i] // per) for i in range(nk) if cnt[i]}


def child(a):
  import numpy as np
  import torch
  import bench
  from dynibar_amd import _lib, engine, render_image
  from frame_case import FrameCase
  assert torch.cuda.is_available(), 'enginebench needs an MI355X (there is no CPU path)'
  lib = _lib.lib()
  check_chains([lib.dyn_profile_name(i).decode() for i in range(lib.dyn_profile_count())])
  res = dict(engine=engine.current())
  step = bench.StaticStep('cuda:0', 4096, 64, 8)
  for _ in range(a.warmup):
    out = step.step()
  torch.cuda.synchronize()
  rounds = []
  for _ in range(3):  # three timed rounds: the spread is printed next to the median
    t0 = time.perf_counter()
    for _ in range(a.steps):
      out = step.step()
    torch.cuda.synchronize()
    rounds.append((time.perf_counter() - t0) / a.steps * 1e3)
  res['step_ms'] = sorted(rounds)
  lib.dyn_profile_enable(1)
  for _ in range(20):
    step.step()
  res['step_kernels'] = _profile(lib, 20)
  lib.dyn_profile_enable(0)
  np.save(os.path.join(a.dir, f'{a.child}_step_rgb.npy'), out['rgb'].float().cpu().numpy())
  fc = FrameCase('cuda:0', 288, 512, 7, 11, 8192)
  frames = []
  for f in range(a.frames + 1):  # (the first frame packs the weights and sizes the workspaces)
    smp, rb = fc.sampler()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ret = fc.render(smp, rb)
    torch.cuda.synchronize()
    frames.append((time.perf_counter() - t0) * 1e3)
  res['frame_ms'] = sorted(frames[1:])
  res['chunk_streams'] = render_image.CHUNK_STREAMS
  render_image.CHUNK_STREAMS = 1
  lib.dyn_profile_enable(1)
  smp, rb = fc.sampler()
  fc.render(smp, rb)
  res['frame_kernels'] = _profile(lib, 1)
  lib.dyn_profile_enable(0)
  np.save(os.path.join(a.dir, f'{a.child}_frame_rgb.npy'), ret['outputs_fine_ref']['rgb'].float().cpu().numpy())
  with open(os.path.join(a.dir, f'{a.child}.json'), 'w') as f:
    json.dump(res, f)


def check_chains(slots):
  """Every chain member must be a profile slot the library has: a renamed slot would otherwise drop out of the sums without a word."""
  unknown = sorted({m for members in CHAINS.values() for m in members} - set(slots))
  if unknown:
    raise SystemExit(f'enginebench: the library has no profile slot named {", ".join(unknown)} (dyn_profile_name): CHAINS is out of date')


def _chain(kernels, names):
  got = [v['ms'] for k, v in kernels.items() if k in names]
  if not got:
    raise SystemExit(f'enginebench: none of {", ".join(names)} was launched: the chain sum would be empty')
  return sum(got)


def report(results, diffs):
  med = lambda xs: xs[len(xs) // 2]
  lines = []
  for name, r in results.items():
    e = r['engine']
    lines.append(f'{name:6s} ({os.path.basename(e["path"])}, {e["terms"]} product(s), kind {e["kind"]}): step {med(r["step_ms"]):.3f} ms (rounds {r["step_ms"][0]:.3f} .. {r["step_ms"][-1]:.3f}), '
                 f'frame {med(r["frame_ms"]):.1f} ms ({r["frame_ms"][0]:.1f} .. {r["frame_ms"][-1]:.1f}, {r["chunk_streams"]} chunk streams)')
  for what in ('step_kernels', 'frame_kernels'):
    lines.append(f'-- {what.replace("_", " ")}: ms per {"step" if what.startswith("step") else "frame"} (launches)' + ''.join(f' | {n}' for n in results) +
                 (' | half / split' if 'half' in results and 'split' in results else ''))
    names = sorted({k for r in results.values() for k in r[what]}, key=lambda k: -max(r[what].get(k, dict(ms=0))['ms'] for r in results.values()))
    for k in names:
      row = f'  {k:26s}'
      for r in results.values():
        v = r[what].get(k)
        row += f' | {v["ms"]:9.3f} ({v["launches"]:4d})' if v else ' |         -       '
      if 'half' in results and 'split' in results and k in results['half'][what] and k in results['split'][what]:
        row += f' | {results["half"][what][k]["ms"] / results["split"][what][k]["ms"]:.3f}'
      lines.append(row)
    for chain, members in chains_of(what.split('_')[0]).items():
      tot = {n: _chain(r[what], members) for n, r in results.items()}
      row = f'  {chain + " (sum)":26s}' + ''.join(f' | {tot[n]:9.3f}       ' for n in results)
      if 'half' in tot and 'split' in tot and tot['split'] > 0:
        row += f' | {tot["half"] / tot["split"]:.3f}'
      lines.append(row)
  def against(a, b):
    x, y = results[a], results[b]
    return (f'{a} / {b}: step {med(x["step_ms"]) / med(y["step_ms"]):.3f}, frame {med(x["frame_ms"]) / med(y["frame_ms"]):.3f}' + ''.join(
        f', {chain} of the {what} {_chain(x[what + "_kernels"], m) / _chain(y[what + "_kernels"], m):.3f}' for what in ('step', 'frame') for chain, m in chains_of(what).items()))
  for name in results:
    if name != 'split' and 'split' in results:
      lines.append(against(name, 'split'))
    if name not in ('split', 'half', 'exact') and 'half' in results:
      lines.append(against(name, 'half'))
  for k, v in diffs.items():
    lines.append(f'max |rgb| difference, {k}: {v:.3e}')
  return '\n'.join(lines)


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--exact', action='store_true', help='also run the 6-term build')
  ap.add_argument('--lib', action='append', default=[], metavar='TAG=PATH', help='one more column: a developer build of the library (repeatable)')
  ap.add_argument('--note', default=None, help='a line for the head of the table (what a --lib build was compiled with)')
  ap.add_argument('--steps', type=int, default=200)
  ap.add_argument('--warmup', type=int, default=20)
  ap.add_argument('--frames', type=int, default=2)
  ap.add_argument('--timeout', type=int, default=240, help='seconds per child')
  ap.add_argument('--out', default=None, help='also write the table to this file')
  ap.add_argument('--child', default=None, help='(internal) the flavour this process measures')
  ap.add_argument('--dir', default=None, help='(internal) where the child leaves its numbers')
  a = ap.parse_args()
  if a.child:
    return child(a)
  import numpy as np
  from dynibar_amd import _lib  # (binding the header only: the parent loads no library and opens no GPU)
  d = tempfile.mkdtemp(prefix='enginebench_')
  results = {}
  flavours = [(n, _lib.engine_path(n)) for n in ['split', 'half'] + (['exact'] if a.exact else [])]
  for spec in a.lib:
    tag, _, path = spec.partition('=')
    if not tag or not path or tag in dict(flavours):
      raise SystemExit(f'--lib {spec}: expected TAG=PATH with a tag of its own')
    flavours.append((tag, os.path.abspath(path)))
  for name, path in flavours:
    if not os.path.exists(path):
      raise SystemExit(f'{path} is missing: python -m dynibar_amd.build')
    env = {k: v for k, v in os.environ.items() if k != 'DYNIBAR_ENGINE'}
    env['DYNIBAR_HIP_LIB'] = path
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child', name, '--dir', d, '--steps', str(a.steps), '--warmup', str(a.warmup),
           '--frames', str(a.frames)]
    print(f'[{name}] {" ".join(cmd[4:])}', flush=True)
    rc = subprocess.run(cmd, env=env).returncode
    if rc != 0:  # nothing more is started on the GPU after a child that failed, faulted or ran into its time limit
      raise SystemExit(f'the {name} child ended with status {rc}: the run ends here')
    results[name] = json.load(open(os.path.join(d, f'{name}.json')))
  diffs = {}
  for other in [n for n in results if n != 'split']:
    for what in ('step', 'frame'):
      x, y = np.load(os.path.join(d, f'split_{what}_rgb.npy')), np.load(os.path.join(d, f'{other}_{what}_rgb.npy'))
      diffs[f'{other} against split, {what} ({x.shape[0] if what == "step" else x.shape[0] * x.shape[1]} rays)'] = float(np.abs(x - y).max())
  txt = report(results, diffs)
  print(txt)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(f'## python tools/enginebench.py{" --exact" if a.exact else ""}{"".join(" --lib " + x for x in a.lib)} --steps {a.steps} --frames {a.frames}   (one session, one child process per flavour)\n' + (f'## {a.note}\n' if a.note else '') + txt + '\n')
  print(json.dumps(dict(metric='engine_flavours', results={n: dict(step_ms=r['step_ms'], frame_ms=r['frame_ms']) for n, r in results.items()}, rgb_differences=diffs)))


if __name__ == '__main__':
  main()
