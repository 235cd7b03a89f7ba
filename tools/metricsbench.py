"""The six numbers of one evaluation frame (eval_nvidia.py:383-457 without LPIPS) at 288 x 512: the host form against dynibar_amd.metrics.
GPU only -- there is no CPU path.

  python tools/metricsbench.py [--seconds 1.0] [--rounds 5]   # one JSON line
  python tools/metricsbench.py --rocprof profiles/metrics_kernel_stats.txt
        # 20 frames in a child process under rocprofv3 --kernel-trace --memory-copy-trace --stats, summarised by tools/rocpd_summary.py

(a) the host form -- what a user of the package did before dynibar_amd.metrics existed: the pixels are on the host (render_image's output
contract), the valid mask and the three calculate_psnr / calculate_ssim pairs run in numpy, the SSIM map through the float64 restatement of
skimage's algorithm with scipy.ndimage.uniform_filter (tests/metrics_restatement.py (A); skimage itself is not installed) and, as the script
does, once per mask.  Its threads are left at the machine's setting.
(b) nvidia_frame_metrics on the same host frame (the upload included) and (c) on a frame that is already on the device.
The forms are timed alternating in the same process after warm-up, device-synchronised, in rounds of at least --seconds each; the spread
over the rounds is reported next to the median.  No speed-up is fixed in advance: the ratios are against (a) on the same machine.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

H, W = 288, 512
NAMES = ('psnr', 'ssim', 'dynamic_psnr', 'dynamic_ssim', 'static_psnr', 'static_ssim')


def seeded_frame():
  import metrics_restatement as mr
  c = mr.make_case(H, W, 'noisy', seed=11)
  return c['pred'], c['target_u8'], c['masks']['dynamic']


def host_form(pred, target_u8, dynamic, R):
  """(:383-457) in numpy / scipy, the SSIM map recomputed for every mask as the script's three calculate_ssim calls do"""
  import numpy as np
  import metrics_restatement as mr
  a, b, valid = mr.prepare(pred, target_u8)
  out = {}
  for prefix, m in (('', valid), ('dynamic_', dynamic), ('static_', 1 - dynamic)):
    S = mr.ssim_map_uniform(b, a, R)
    out[prefix + 'ssim'] = float(np.sum(S * m) / (np.sum(m) + 1e-8))
    out[prefix + 'psnr'] = mr.calculate_psnr_restated(b, a, m)
  return out


def _stats(xs):
  xs = sorted(xs)
  return dict(median_ms=round(xs[len(xs) // 2], 4), min_ms=round(xs[0], 4), max_ms=round(xs[-1], 4))


def alternate(fs, seconds, rounds, warmup=3):
  """time the callables alternating: per round each runs for at least `seconds`, synchronised at both ends -> per-call ms of every round"""
  import torch
  for _ in range(warmup):
    for f in fs:
      f()
  torch.cuda.synchronize()
  out = [[] for _ in fs]
  for _ in range(rounds):
    for f, dst in zip(fs, out):
      n, t0 = 0, time.perf_counter()
      while True:
        for _ in range(5):
          f()
        n += 5
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
          break
      dst.append(dt / n * 1e3)
  return out


def run(seconds, rounds):
  import torch
  from dynibar_amd import _lib, metrics
  assert torch.cuda.is_available(), 'metricsbench needs an MI355X (there is no CPU path)'
  _lib.lib()
  R = metrics.REFERENCE_DATA_RANGE
  pred, tgt, dyn = seeded_frame()
  pred_h, tgt_h, dyn_h = torch.from_numpy(pred), torch.from_numpy(tgt), torch.from_numpy(dyn)
  pred_d, tgt_d, dyn_d = pred_h.cuda(), tgt_h.cuda(), dyn_h.cuda()
  host = lambda: host_form(pred, tgt, dyn, R)
  up = lambda: metrics.nvidia_frame_metrics(pred_h, tgt_h, dyn_h)
  dev = lambda: metrics.nvidia_frame_metrics(pred_d, tgt_d, dyn_d)
  a, b, c = host(), up(), dev()
  assert b == c, (b, c)
  worst = max(abs(a[k] - b[k]) for k in NAMES)
  assert worst < 1e-9, (a, b)
  th, tu, td = alternate((host, up, dev), seconds, rounds)
  sh, su, sd = _stats(th), _stats(tu), _stats(td)
  return dict(metric='frame_metrics_ms', shape=f'{H}x{W}', data_range=R, seconds_per_round=seconds, rounds=rounds, host_threads=torch.get_num_threads(),
              host_form=sh, device_form_host_frame=su, device_form_device_frame=sd, ratio_host_frame=round(sh['median_ms'] / su['median_ms'], 2),
              ratio_device_frame=round(sh['median_ms'] / sd['median_ms'], 2), max_abs_difference_of_the_six_numbers=worst, numbers=b)


def profile(path):
  import glob
  import sqlite3
  import tempfile
  frames = 20
  d = tempfile.mkdtemp(prefix='metricsbench_')
  cmd = ['timeout', '-k', '10', '300', 'rocprofv3', '--kernel-trace', '--memory-copy-trace', '--stats', '-d', d, '--', sys.executable,
         os.path.abspath(__file__), '--only', str(frames)]
  subprocess.run(cmd, check=True, cwd=d)  # (a failure ends the tool: nothing more is started on the GPU)
  dbs = sorted(glob.glob(os.path.join(d, '**', '*.db'), recursive=True))
  assert dbs, f'rocprofv3 wrote no database under {d}'
  txt = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rocpd_summary.py'), 'stats', dbs[0]], check=True, capture_output=True,
                       text=True).stdout.replace(d, '<run dir>')
  rows = [l for l in txt.splitlines()[2:] if l.strip()]
  calls = sum(int(l.split()[-13]) for l in rows)
  ours = sum(int(l.split()[-13]) for l in rows if l.startswith('k_metrics'))
  cur = sqlite3.connect(dbs[0]).cursor()
  names = [r[0] for r in cur.execute("select name from sqlite_master where type in ('table', 'view') and name like '%memory_cop%'")]
  copies = 'not recorded (no memory-copy table in the database)'
  for n in sorted(names, key=len):
    try:
      copies = f'{cur.execute(f"select count(*) from {n}").fetchone()[0]} in all ({n}; the {3} uploads of the frame once, then per frame the copy of the sums)'
      break
    except sqlite3.Error:
      continue
  head = (f'## python tools/metricsbench.py --only {frames}  ({frames} frames of nvidia_frame_metrics at {H} x {W} on a device frame, after the upload)\n'
          f'## kernel launches: {calls} = {calls / frames:.1f} per frame, of which k_metrics_*: {ours} = {ours / frames:.1f} per frame (the rest is the mask '
          f'preparation and scratch fill on torch)\n## memory copies: {copies}\n')
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, 'w') as f:
    f.write(head + txt)
  print(head + txt)


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--seconds', type=float, default=1.0)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--rocprof', default=None, help='write the rocprofv3 kernel stats of a separate run to this file')
  ap.add_argument('--only', type=int, default=0, help='(internal: the child runs under the profiler) this many frames of the device form')
  a = ap.parse_args()
  if a.only:
    import torch
    from dynibar_amd import metrics
    pred, tgt, dyn = (torch.from_numpy(x).cuda() for x in seeded_frame())
    for _ in range(a.only):
      metrics.nvidia_frame_metrics(pred, tgt, dyn)
    torch.cuda.synchronize()
    return
  if a.rocprof:
    return profile(a.rocprof)
  print(json.dumps(run(a.seconds, a.rounds)))


if __name__ == '__main__':
  main()
