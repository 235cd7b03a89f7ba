"""The three LPIPS numbers of one evaluation frame (eval_nvidia.py:402-457) at 288 x 512 with three masks: the device call against the host form.
GPU only -- there is no CPU path.

  python tools/lpipsbench.py [--seconds 1.0] [--rounds 5]   # one JSON line

(a) the device call: ``net.frame_sums`` on a frame that is already on the device (the renderer's ``frame_outputs='device'``) with the masks
valid, dynamic and static, and the copy of its ``[3, 5, 2]`` table to the host -- what ``nvidia_eval`` queues per view.
(b) the host form -- what a user of the package did before dynibar_amd.lpips existed: the pixels are on the host, the valid mask and the masked
images are rebuilt in numpy, and the same network (tests/lpips_restatement.py's layers and random weights, torch on the same GPU, float32) runs
three times, once per mask, each time on both images copied from the host, with the masked average of the package's stated form and one
``.item()`` per mask.  The script's own ``models`` package was not available: this is the same arithmetic on torch, not that package.
The forms are timed alternating in the same process after warm-up, device-synchronised, in rounds of at least --seconds each.  No speed-up is
fixed in advance.  Synthetic random weights: the time does not depend on their values.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

H, W = 288, 512


def _stats(xs):
  xs = sorted(xs)
  return dict(median_ms=round(xs[len(xs) // 2], 4), min_ms=round(xs[0], 4), max_ms=round(xs[-1], 4))


def alternate(fs, seconds, rounds, warmup=3):
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
  import numpy as np
  import torch
  import torch.nn.functional as F
  import lpips_restatement as lr
  from dynibar_amd import _lib, lpips
  assert torch.cuda.is_available(), 'lpipsbench needs an MI355X (there is no CPU path)'
  _lib.lib()
  dev = torch.device('cuda', 0)
  weights = lr.random_weights(0)
  net = lpips.LPIPS(*weights)
  pred, tgt = lr.make_pair(H, W, 'border', 3)
  dyn = lr.make_masks(H, W)['dynamic']
  pred_d, tgt_d = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
  masks_d = torch.from_numpy(np.stack([dyn, 1 - dyn])).to(dev).contiguous()
  alex = {k: v.to(dev) for k, v in weights[0].items()}
  lin = [weights[1][f'lin{l}.model.1.weight'].to(dev) for l in range(5)]

  def device_form():
    rows = net.frame_sums(pred_d, tgt_d, masks_d, apply_valid=True, valid_as_mask0=True)['sums'].cpu().tolist()
    return [lpips.lpips_of(t) for t in rows]

  def host_form():
    valid = np.float32(np.sum(pred, axis=-1, keepdims=True) > 1e-3)
    a, b = pred * valid, (np.float32(tgt) / 255) * valid
    out = []
    for m in (valid, dyn, 1 - dyn):
      with torch.no_grad():
        x = torch.stack([torch.from_numpy(q / np.float32(0.5) - np.float32(1)).to(dev) for q in (a, b)]).permute(0, 3, 1, 2)  # im2tensor(...).cuda()
        x = (x - torch.tensor(lr.SHIFT, device=dev).view(1, 3, 1, 1)) / torch.tensor(lr.SCALE, device=dev).view(1, 3, 1, 1)
        mk = torch.from_numpy(np.ascontiguousarray(m[..., 0])).to(dev)[None, None]
        total = 0.0
        for l, f in enumerate(lr.features(x, alex, torch.float32)):
          n = f / (torch.sqrt(torch.sum(f * f, dim=1, keepdim=True)) + 1e-10)
          d = torch.sum(lin[l] * (n[0:1] - n[1:2]) ** 2, dim=1, keepdim=True)
          ml = F.interpolate(mk, size=d.shape[2:], mode='nearest')
          s = ml.sum()
          total = total + torch.where(s > 0, (d * ml).sum() / s.clamp_min(1e-30), torch.zeros_like(s))
        out.append(float(total.item()))
    return out

  a, b = device_form(), host_form()
  worst = max(abs(x - y) / max(abs(y), 1e-30) for x, y in zip(a, b))
  assert worst < 1e-3, (a, b)
  td, th = alternate((device_form, host_form), seconds, rounds)
  sd, sh = _stats(td), _stats(th)
  # the per-kernel split of the device call (HIP events around every launch)
  import ctypes
  lib = _lib.lib()
  n = lib.dyn_profile_count()
  ms, launches = (ctypes.c_float * n)(), (ctypes.c_int * n)()
  lib.dyn_profile_enable(1)
  lib.dyn_profile_read(ms, launches)
  frames = 20
  for _ in range(frames):
    device_form()
  torch.cuda.synchronize()
  lib.dyn_profile_read(ms, launches)
  lib.dyn_profile_enable(0)
  prof = {lib.dyn_profile_name(i).decode(): dict(ms=round(ms[i] / frames, 4), launches=launches[i] // frames) for i in range(n) if launches[i]}
  return dict(metric='lpips_frame_ms', shape=f'{H}x{W}', masks=3, seconds_per_round=seconds, rounds=rounds, device_call=sd, host_form=sh,
              ratio=round(sh['median_ms'] / sd['median_ms'], 2), kernel_ms_per_frame=prof, max_rel_difference_of_the_three_numbers=worst, numbers=a)


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--seconds', type=float, default=1.0)
  ap.add_argument('--rounds', type=int, default=5)
  a = ap.parse_args()
  print(json.dumps(run(a.seconds, a.rounds)))


if __name__ == '__main__':
  main()
