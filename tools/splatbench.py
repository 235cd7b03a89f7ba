"""GPU time of the virtual source views of one frame (8 views at 288 x 512, B = 8 in one batched call): dynibar_amd.virtual_views.
GPU only -- there is no CPU path.

  python tools/splatbench.py [--frames 20] [--warmup 5]     # per-frame device time, per-pass times and bytes, one JSON line
  python tools/splatbench.py --rocprof profiles/vv_splat_kernel_stats.txt
        # the same loop in a child process under rocprofv3 --kernel-trace --stats, summarised by tools/rocpd_summary.py

Per frame: k_sobel_alpha, the forward splat (k_splat_project, k_splat_keys, the radix passes, k_splat_bounds, k_splat_resolve) and
k_vv_finish.  The frame's inputs are staged on the device once (plumbing, not timed); the timed region is what
render_frame_virtual_views launches.  Bytes per pass are the algorithmic bytes of dyn_splat.h's data flow (every array read or written
once; gathers priced at their element size), against 8 TB/s of HBM.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8e12


def byte_model(B, H, W, C=4):
  """Algorithmic bytes per pass of one batched call (see dyn_splat.h)."""
  N = B * H * W
  M = 4 * N
  bits = N.bit_length()
  passes = (bits + 7) // 8
  ntiles = -(-M // 4096)
  hist = 256 * ntiles * 4
  sort = 0
  for p in range(passes):
    sort += M * 4 + hist  # histogram: keys in, tile histograms out
    sort += 2 * hist      # scan (in place)
    sort += M * 4 * (1 if p == 0 else 2) + M * 8  # scatter: keys (+ ids after the first pass) in, keys + ids out
  cout = C + 2
  groups = -(-cout // 4)
  per_contrib = 4 + 8 + 4  # id, flow (2 floats), multiplier
  resolve = groups * (N * 8 + M * (per_contrib + 4 * min(4, cout))) + N * cout * 4  # per channel group: bounds, then the listed sources
  return {
      'k_sobel_alpha': N // B * 4 * 2,
      'k_splat_project': N * (4 + 8 + 4),
      'k_splat_keys': N * (8 + 4 + 4 + 16 + 8),
      'k_splat_sort': sort + M * 4 + N * 8,  # (+ k_splat_bounds: sorted keys in, bounds out)
      'k_splat_resolve': resolve,
      'k_vv_finish': N * (4 * 4 + 3),
      'radix_passes': passes,
  }


def run(frames, warmup, profile_slots):
  import numpy as np
  import torch
  from dynibar_amd import _lib, virtual_views as vv
  assert torch.cuda.is_available(), 'splatbench needs an MI355X (there is no CPU path)'
  lib = _lib.lib()
  H, W = 288, 512
  rng = np.random.RandomState(0)
  yy, xx = np.mgrid[0:H, 0:W]
  img = np.clip(0.5 + 0.4 * np.sin(xx / 17.0)[..., None] * np.cos(yy[..., None] / 11.0 + np.arange(3)), 0, 1).astype(np.float32)
  disp = (0.3 + 0.15 * np.sin(xx / 53.0) * np.cos(yy / 31.0) + 0.05 * rng.uniform(size=(H, W))).astype(np.float32)
  f = 0.9 * W
  K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
  c2w = np.eye(4)
  _, vsv = vv.virtual_view_poses([c2w.astype(np.float32)], [1.0 / disp.max()], np.array([H, W, f]).reshape([3, 1]))
  dev = torch.device('cuda:0')
  img_d, disp_d = torch.from_numpy(img).to(dev), torch.from_numpy(disp).to(dev)

  def frame():
    with torch.no_grad():
      src, depth, rot, t, k = vv.frame_batch(img_d, disp_d, K, c2w, vsv[0])  # k_sobel_alpha and the staging of the batch
      o = vv.forward_splat(src, depth, rot, t, k, k)
      return vv.vv_finish(o['feat'])

  for _ in range(warmup):
    frame()
  torch.cuda.synchronize()
  ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(frames)]
  t0 = time.perf_counter()
  for a, b in ev:
    a.record()
    frame()
    b.record()
  torch.cuda.synchronize()
  wall = (time.perf_counter() - t0) / frames
  ms = sorted(a.elapsed_time(b) for a, b in ev)
  out = {'metric': 'vv_frame_ms', 'B': 8, 'H': H, 'W': W, 'frames': frames, 'frame_ms_median': ms[len(ms) // 2], 'frame_ms_min': ms[0],
         'frame_wall_ms': wall * 1e3, 'target_ms': 0.1}
  if profile_slots:
    lib.dyn_profile_enable(1)
    nk = lib.dyn_profile_count()
    tot, cnt = (ctypes.c_float * nk)(), (ctypes.c_int * nk)()
    lib.dyn_profile_read(tot, cnt)  # reset
    for _ in range(frames):
      frame()
    torch.cuda.synchronize()
    lib.dyn_profile_read(tot, cnt)
    lib.dyn_profile_enable(0)
    lib.dyn_profile_name.restype = ctypes.c_char_p
    model = byte_model(8, H, W)
    passes = {}
    for i in range(nk):
      name = lib.dyn_profile_name(i).decode()
      if cnt[i] and name in model:
        t_ms = tot[i] / frames
        passes[name] = {'ms': round(t_ms, 4), 'launches_per_frame': cnt[i] // frames, 'MB': round(model[name] / 1e6, 2),
                        'frac_of_8TBps': round(model[name] / (t_ms * 1e-3) / HBM, 3)}
    out['passes'] = passes
    out['radix_passes'] = model['radix_passes']
    out['model_MB_per_frame'] = round(sum(v for k_, v in model.items() if k_.startswith('k_')) / 1e6, 1)
  return out


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--frames', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--rocprof', default=None, help='write the rocprofv3 kernel stats of a separate run to this file')
  ap.add_argument('--no-slots', action='store_true', help='(internal: the child run under the profiler)')
  a = ap.parse_args()
  if a.rocprof:
    import glob
    import tempfile
    d = tempfile.mkdtemp(prefix='splatbench_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', d, '--', sys.executable, os.path.abspath(__file__), '--frames', str(a.frames),
           '--warmup', str(a.warmup), '--no-slots']
    subprocess.run(cmd, check=True, cwd=d, timeout=600)
    dbs = sorted(glob.glob(os.path.join(d, '**', '*.db'), recursive=True))
    assert dbs, f'rocprofv3 wrote no database under {d}'
    txt = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rocpd_summary.py'), 'stats', dbs[0]], check=True, capture_output=True,
                         text=True).stdout
    os.makedirs(os.path.dirname(os.path.abspath(a.rocprof)), exist_ok=True)
    with open(a.rocprof, 'w') as f:
      f.write(f'# python tools/splatbench.py --frames {a.frames} --warmup {a.warmup} (8 virtual views of a 288 x 512 frame per iteration)\n')
      f.write(txt.replace(d, '<run dir>'))
    print(txt)
    return
  print(json.dumps(run(a.frames, a.warmup, not a.no_slots)))


if __name__ == '__main__':
  main()
