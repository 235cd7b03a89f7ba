"""Flow supervision of a whole scene at the frame size (60 frames of 288 x 512): dynibar_amd.flow_prep.supervision, one launch of
k_flow_supervision with masks, epi and motion.  GPU only -- there is no CPU path.

  python tools/flowprepbench.py [--frames 60] [--repeats 5] [--calls 20] [--out profiles/flow_prep.txt]

The kernel is a gather with a stated traffic model, computed here from the shapes: per pixel of a frame 48 B of own flow read (six
float2), plus four 8 B taps of each of six partner flows that lie within a few pixels of the lane's own position and are counted as cache
hits, and 6 B of masks + 24 B of epi + 1 B of motion written: 79 B per pixel from and to memory.  The time is printed next to that byte count
divided by 8 TB/s, the memory bandwidth of the MI355X.  There is no pass / fail threshold: the number is a report.

After a warm-up (the first launch loads the code object), each of ``--repeats`` windows times ``--calls`` back-to-back calls with device events
and divides; the median, the least and the largest window are printed, so the spread is visible.  The inputs are seeded smooth flows of
3 px; the share of ones in the masks and in the motion vote is reported so that a reader sees the check was exercised.  The outputs are not
compared with the restatement here (tests/test_gpu_flow_prep.py does that)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

H, W = 288, 512
READ_BYTES, WRITE_BYTES = 6 * 8, 6 * 1 + 6 * 4 + 1  # per pixel of a frame: own flow in; masks, epi and motion out
PEAK_BYTES_PER_S = 8e12


def model_bytes(frames, h=H, w=W):
  return frames * h * w * (READ_BYTES + WRITE_BYTES)


def run(frames, repeats, calls):
  import numpy as np
  import torch
  import flow_prep_cases as fc
  from dynibar_amd import flow_prep
  if not torch.cuda.is_available():
    raise SystemExit('flowprepbench needs an MI355X: there is no CPU path and no number without one')
  dev = 'cuda:0'
  rng = np.random.default_rng(7)
  base = np.stack([fc.smooth(rng, H, W, 3.0) for _ in range(6)]).astype(np.float32)  # six fields, shifted from frame to frame
  flows = torch.from_numpy(np.stack([np.roll(base, 5 * i, axis=2) for i in range(frames)])).to(dev)
  flows[:, 3:] = -flows[:, :3] + 0.3
  K, c2w = fc.scene_cameras(frames, H, W)
  F = torch.from_numpy(flow_prep.fundamental_matrices(K, c2w)).to(dev)
  masks = torch.empty((frames, 6, H, W), dtype=torch.uint8, device=dev)
  epi = torch.empty((frames, 6, H, W), dtype=torch.float32, device=dev)
  motion = torch.empty((frames, H, W), dtype=torch.uint8, device=dev)

  def call():
    flow_prep._launch(flows, frames, H, W, F, 0.5, 0.5, 32, 1.0, 2, masks, epi, motion)

  for _ in range(3):
    call()
  torch.cuda.synchronize()
  ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  ms = []
  for _ in range(repeats):
    ev0.record()
    for _ in range(calls):
      call()
    ev1.record()
    torch.cuda.synchronize()
    ms.append(ev0.elapsed_time(ev1) / calls)
  ones = float(masks.float().mean())
  nbytes = model_bytes(frames)
  floor_ms = nbytes / PEAK_BYTES_PER_S * 1e3
  med = statistics.median(ms)
  return dict(frames=frames, shape=[H, W], repeats=repeats, calls_per_window=calls, call_ms=dict(median=round(med, 4), min=round(min(ms), 4), max=round(max(ms), 4)),
              model_bytes=nbytes, bytes_over_8TBps_ms=round(floor_ms, 4), model_share_of_peak_bandwidth=round(floor_ms / med, 3),
              achieved_model_TBps=round(nbytes / (med * 1e-3) / 1e12, 3), mask_ones=round(ones, 3), motion_ones=round(float(motion.float().mean()), 3),
              device=torch.cuda.get_device_name(0))


def main():
  ap = argparse.ArgumentParser(description='Time flow_prep.supervision at the frame size next to its traffic model (GPU only).')
  ap.add_argument('--frames', type=int, default=60)
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  line = json.dumps(run(a.frames, a.repeats, a.calls))
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
