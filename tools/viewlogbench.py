"""The training loop's logged view panels at the frame size (288 x 512, 6 + 6 flows): dynibar_amd.view_log.panels + .cpu() on the device
against the host path it replaces, in one process on the same tensors.  GPU only -- there is no CPU path.

  python tools/viewlogbench.py [--rounds 20] [--out profiles/view_log.txt]

(a) the device path: three launches (k_viewlog_ranges, k_viewlog_flow_max, k_viewlog_panels) into the packed buffer and ONE pinned copy to the
host; timed by the host clock around work that ends in a stream synchronise, and per kernel by the library's event times in a separate pass.
(b) the host path: the device-to-host copies of the frame's groups that log_view_to_tb makes (train.py:657-678, :736-742), then the numpy
restatement of its images (tests/view_log_cases.py: equal to the real colorize / flow_to_image bit for bit).  The restatement does NOT draw
the matplotlib colour-bar figure that the real colorize draws and throws away with append_cbar=False, so (b) is a lower bound of what the
script spends.  Both alternate after a warm-up; the panels of (a) are compared with (b) exactly before anything is timed.  No ratio is fixed
in advance."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

H, W, N_FLOWS = 288, 512, 6


def run(rounds):
  import numpy as np
  import torch
  import view_log_cases as vc
  from dynibar_amd import _lib, view_log
  dev = 'cuda:0'
  ret, gt_img, gt_disp, gt_flows = vc.synthetic_groups(H, W, N_FLOWS)
  ret['outputs_coarse_anchor']['depth'] = ret['outputs_coarse_ref']['depth'].clone()  # (copied by the script, :677, and never used)
  dret = vc.to_device(ret, dev)
  dgt = gt_img.to(dev), gt_disp.to(dev), gt_flows.to(dev)

  def device_path():
    return view_log.panels(dret, *dgt).cpu()

  def host_path():
    host = {g: {k: v.detach().cpu() for k, v in grp.items()} for g, grp in dret.items()}
    return vc.panels_restated(host, dgt[0].cpu(), dgt[1].cpu(), dgt[2].cpu())

  got, want = device_path(), host_path()
  for tag in view_log.TAGS:
    vc.assert_same(got[tag], want[tag].contiguous(), tag)
  dev_ms, host_ms = [], []
  for r in range(rounds + 2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    device_path()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    host_path()
    t2 = time.perf_counter()
    if r >= 2:
      dev_ms.append((t1 - t0) * 1e3)
      host_ms.append((t2 - t1) * 1e3)
  lib = _lib.lib()
  n = lib.dyn_profile_count()
  ms, cnt = np.zeros(n, np.float32), np.zeros(n, np.int32)
  lib.dyn_profile_enable(1)
  lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
  for _ in range(rounds):
    view_log.panels(dret, *dgt)
  torch.cuda.synchronize()
  lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
  lib.dyn_profile_enable(0)
  kernel_ms = {lib.dyn_profile_name(i).decode(): round(float(ms[i]) / int(cnt[i]), 5) for i in range(n) if cnt[i]}
  ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  copy_ms = []
  p = view_log.panels(dret, *dgt)
  for _ in range(rounds):
    torch.cuda.synchronize()
    ev0.record()
    p.cpu()
    ev1.record()
    torch.cuda.synchronize()
    copy_ms.append(ev0.elapsed_time(ev1))
  q = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
  return dict(shape=[H, W], flows=[N_FLOWS, N_FLOWS], rounds=rounds, packed_bytes=int(p.buffer.numel()), device_path_ms=q(dev_ms), host_path_ms=q(host_ms),
              kernel_ms=kernel_ms, kernels_sum_ms=round(sum(kernel_ms.values()), 5), copy_ms=q(copy_ms), exact=True,
              device=torch.cuda.get_device_name(0), numpy=np.__version__)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=20)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  line = json.dumps(run(a.rounds))
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
