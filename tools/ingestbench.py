"""Scene preparation at the user's sizes: each dynibar_amd.ingest operation against the torch form of the same operation on the same GPU, in one
process, alternating.  GPU only -- there is no CPU path.

  python tools/ingestbench.py [--rounds 20] [--batch 8] [--out profiles/ingest.txt]
  python tools/ingestbench.py --rocprof profiles/ingest_kernel_stats.txt     # kernel times: a separate run under rocprofv3 --kernel-trace --stats
  python tools/ingestbench.py --virtual_views [--out profiles/ingest_virtual_views.txt]      # 16 frames x 8 views at 288 x 512: the per-frame
      path (render_frame_virtual_views with its copy to the host) against ingest.virtual_views at batch 8 and 16, inputs on the device, median
      of 5 runs after 2 warm-ups, a host clock around work that ends in a stream synchronise; the bytes are compared first
  python tools/ingestbench.py --virtual_views --rounds 5 --rocprof profiles/ingest_virtual_views_kernel_stats.txt    # its kernels, a separate run

Seeded inputs: frames 1080 x 1920 x 3 -> 288 x 512 (area), depth 384 x 672 -> 288 x 512 (linear), masks 1080 x 1920 -> 288 x 512 (nearest),
erosion with r = 3 and depth bounds (5, 95) at 384 x 672, `batch` images per call.  After a warm-up each round times the ingest call and then
the torch form with device events around work that ends in a synchronise.  The torch forms: F.interpolate area / bilinear / nearest (float
tensors in torch's NCHW layout, converted outside the timed window), -max_pool2d(-x) per row chord of the disk, torch.quantile.  They do
not compute the same bits (F.interpolate is not cv2's arithmetic): they are the same operation by the user's meaning, on the same device.
The share of the HBM peak is computed from the algorithmic bytes -- the source read once, the destination written once -- over the kernel
time of the --rocprof run (or, without one, over the call time, which includes the launch).  No ratio is fixed in advance."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HS, WS, H, W = 1080, 1920, 288, 512
HD, WD = 384, 672
RADIUS = 3
HBM_PEAK = 8.0e12  # bytes per second (MI355X, HBM3E)


def torch_erode(x, radius):
  """the disk as the union of its row chords: per chord a horizontal min filter (-max_pool2d(-x)) of the chord's width, read dy rows away;
  taps outside the image count as 1.  x float [B, 1, H, W] of 0 / 1"""
  import torch
  import torch.nn.functional as F
  Hx = x.shape[2]
  out = None
  for dy in range(-radius, radius + 1):
    c = 0
    while (c + 1) ** 2 + dy * dy <= radius * radius:
      c += 1
    row = -F.max_pool2d(F.pad(-x, (c, c, 0, 0), value=-1.0), (1, 2 * c + 1), stride=1)
    row = F.pad(row, (0, 0, radius, radius), value=1.0)[:, :, radius + dy:radius + dy + Hx]
    out = row if out is None else torch.minimum(out, row)
  return out


def cases(batch):
  """name -> (the ingest call, the torch form, algorithmic bytes)"""
  import numpy as np
  import torch
  import torch.nn.functional as F
  import ingest_cases as ic
  from dynibar_amd import ingest
  dev = 'cuda:0'
  frames = ic.dev_t(ic.u8_image(batch, HS, WS, 3, seed=1), dev)
  depth = ic.dev_t(ic.f32_image(batch, HD, WD, seed=1), dev)
  raw = ic.dev_t(ic.raw_mask(batch, HS, WS, seed=1), dev)
  mask = ic.dev_t(ic.mask01(batch, H, W, density=0.98, seed=1), dev)
  frames_f = frames.permute(0, 3, 1, 2).float().contiguous()
  raw_f, mask_f = raw[:, None].float(), mask[:, None].float()
  q = torch.tensor([0.05, 0.95], device=dev)
  return {
      'resize_area': (lambda: ingest.resize_area(frames, (W, H)), lambda: F.interpolate(frames_f, size=(H, W), mode='area'),
                      batch * (HS * WS * 3 + H * W * 3)),
      'resize_linear': (lambda: ingest.resize_linear(depth, (W, H)),
                        lambda: F.interpolate(depth[:, None], size=(H, W), mode='bilinear', align_corners=False), batch * (HD * WD + H * W) * 4),
      'resize_nearest': (lambda: ingest.resize_nearest(raw[..., None], (W, H)), lambda: F.interpolate(raw_f, size=(H, W), mode='nearest'),
                         batch * (HS * WS + H * W)),
      'erode_disk': (lambda: ingest.erode_disk(mask, RADIUS), lambda: torch_erode(mask_f, RADIUS), batch * 2 * H * W),
      'depth_bounds': (lambda: ingest.depth_bounds(depth), lambda: torch.quantile(depth.reshape(batch, -1), q, dim=1), batch * HD * WD * 4),
  }


def run(rounds, batch):
  import numpy as np
  import torch
  ops = cases(batch)
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
  out = dict(batch=batch, rounds=rounds, frames=[HS, WS, H, W], depth=[HD, WD, H, W], radius=RADIUS, device=torch.cuda.get_device_name(0), ops={})
  for name, (ours, theirs, nbytes) in ops.items():
    for _ in range(3):
      ours()
      theirs()
    torch.cuda.synchronize()
    a_ms, b_ms = [], []
    for _ in range(rounds):
      ev[0].record()
      ours()
      ev[1].record()
      theirs()
      ev[2].record()
      torch.cuda.synchronize()
      a_ms.append(ev[0].elapsed_time(ev[1]))
      b_ms.append(ev[1].elapsed_time(ev[2]))
    q = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    out['ops'][name] = dict(ingest_ms=q(a_ms), torch_ms=q(b_ms), algorithmic_bytes=nbytes,
                            hbm_share_of_call=round(nbytes / (statistics.median(a_ms) * 1e-3) / HBM_PEAK, 4))
  return out


def loop(rounds, batch):
  """the ingest calls alone: the child run under the profiler"""
  import torch
  ops = cases(batch)
  for _ in range(rounds):
    for name, (ours, _, _) in ops.items():
      ours()
  torch.cuda.synchronize()


VV_FRAMES, VV_VIEWS, VV_RUNS, VV_WARMUPS = 16, 8, 5, 2


def vv_inputs():
  """16 frames at 288 x 512 on the device with the script's 8 poses each (tests/vv_ingest_cases.py: a smooth image, a disparity with a step; the
  nearest pixel shifts by about 20 px)"""
  import vv_ingest_cases as vc
  import ingest_cases as ic
  img, disp, K, c2w, vsv = vc.vv_inputs(F=VV_FRAMES, H=H, W=W, shift=20.0)
  return ic.dev_t(img, 'cuda:0'), ic.dev_t(disp, 'cuda:0'), K, c2w, vsv


def vv_bytes_per_frame():
  """what the kernels of dyn_vv_frames read and write per frame of 8 views, from the shapes (the sort's passes at 8 frames per call: 3)"""
  hw, v = H * W, VV_VIEWS
  source = hw * (3 * 4 + 9 * 4 + 16)                   # k_vv_source: img, nine disparity taps (cached: counted once each), rgba
  project = v * hw * (4 + 12)                          # disp (once per view), flow + importance
  keys = v * hw * (12 + 16 + 4 + 8)                    # flow + importance, 4 keys, exp(w), list bounds
  sort = 3 * v * hw * 4 * (4 + 8 + 8)                  # per pass and contribution: histogram read, scatter read and write of (key, id)
  bounds = v * hw * 4 * 4 + v * hw * 8
  resolve = v * hw * (8 + 4 * (4 + 8 + 4 + 16) + 4)    # bounds, per contribution id + flow + exp(w) + rgba, the packed pixel
  erode = v * hw * (4 + 3)
  return dict(source=source, project=project, keys=keys, sort=sort, bounds=bounds, resolve=resolve, erode=erode,
              total=source + project + keys + sort + bounds + resolve + erode, old_path_eightfold_fp32_buffers=v * hw * (16 + 4) * 2)


def run_virtual_views():
  """(a) the per-frame path, render_frame_virtual_views for each of the 16 frames with its copy to the host, against (b) ingest.virtual_views with
  batch 8 and 16: median of 5 runs after 2 warm-ups, a host clock around work that ends in a stream synchronise, the legs alternating"""
  import time
  import numpy as np
  import torch
  from dynibar_amd import ingest, virtual_views as vv
  img, disp, K, c2w, vsv = vv_inputs()
  legs = {
      'per_frame': lambda: [vv.render_frame_virtual_views(img[f], disp[f], K, c2w[f], vsv[f]) for f in range(VV_FRAMES)],
      'batch_8': lambda: ingest.virtual_views(img, disp, K, c2w, vsv, batch=8),
      'batch_16': lambda: ingest.virtual_views(img, disp, K, c2w, vsv, batch=16),
  }
  want = np.stack(legs['per_frame']())
  for name in ('batch_8', 'batch_16'):
    assert np.array_equal(legs[name]().cpu().numpy(), want), name  # the bytes of the path it replaces, at the size that is timed
  st = torch.cuda.current_stream()
  times = {k: [] for k in legs}
  for r in range(VV_WARMUPS + VV_RUNS):
    for name, fn in legs.items():
      st.synchronize()
      t0 = time.perf_counter()
      fn()
      st.synchronize()
      if r >= VV_WARMUPS:
        times[name].append((time.perf_counter() - t0) * 1e3)
  q = lambda v: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), runs=[round(x, 3) for x in v])
  out = dict(frames=VV_FRAMES, views=VV_VIEWS, size=[H, W], device=torch.cuda.get_device_name(0), fill=round(float((want.max(-1) > 0).mean()), 3),
             ms={k: q(v) for k, v in times.items()}, bytes_per_frame=vv_bytes_per_frame())
  a = out['ms']['per_frame']
  out['spread_per_frame_ms'] = round(a['max'] - a['min'], 3)
  for name in ('batch_8', 'batch_16'):
    out[f'{name}_over_per_frame'] = round(out['ms'][name]['median'] / a['median'], 4)
  return out


def loop_virtual_views(rounds):
  import torch
  from dynibar_amd import ingest
  img, disp, K, c2w, vsv = vv_inputs()
  for _ in range(rounds):
    ingest.virtual_views(img, disp, K, c2w, vsv, batch=8)
  torch.cuda.synchronize()


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--rounds', type=int, default=20)
  ap.add_argument('--batch', type=int, default=8)
  ap.add_argument('--out', default=None)
  ap.add_argument('--rocprof', default=None, help='write the rocprofv3 kernel stats of a separate run to this file')
  ap.add_argument('--loop', action='store_true', help='(internal: the child run under the profiler)')
  ap.add_argument('--virtual_views', action='store_true',
                  help='the virtual views of 16 frames x 8 views at 288 x 512: the per-frame path against ingest.virtual_views (with --rocprof: the '
                       'kernels of ingest.virtual_views at batch 8)')
  a = ap.parse_args()
  if a.loop:
    loop_virtual_views(a.rounds) if a.virtual_views else loop(a.rounds, a.batch)
    return
  if a.rocprof:
    import glob
    import tempfile
    d = tempfile.mkdtemp(prefix='ingestbench_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', d, '--', sys.executable, os.path.abspath(__file__), '--rounds', str(a.rounds), '--batch',
           str(a.batch), '--loop'] + (['--virtual_views'] if a.virtual_views else [])
    subprocess.run(cmd, check=True, cwd=d, timeout=600)
    dbs = sorted(glob.glob(os.path.join(d, '**', '*.db'), recursive=True))
    assert dbs, f'rocprofv3 wrote no database under {d}'
    txt = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rocpd_summary.py'), 'stats', dbs[0]], check=True, capture_output=True,
                         text=True).stdout
    os.makedirs(os.path.dirname(os.path.abspath(a.rocprof)), exist_ok=True)
    with open(a.rocprof, 'w') as f:
      if a.virtual_views:
        f.write(f'# python tools/ingestbench.py --virtual_views --rounds {a.rounds} --loop ({a.rounds} calls of ingest.virtual_views: {VV_FRAMES} frames '
                f'x {VV_VIEWS} views at {H} x {W}, batch 8)\n')
      else:
        f.write(f'# python tools/ingestbench.py --rounds {a.rounds} --batch {a.batch} --loop ({a.batch} images per call)\n')
      f.write('\n'.join(ln.split('   (')[0] + '   durations in microseconds' if ln.startswith('# rocprofv3') and '.db)' in ln else ln
                        for ln in txt.split('\n')))  # (the summary's header names the run's database file: not kept)
    print(txt)
    return
  line = json.dumps(run_virtual_views() if a.virtual_views else run(a.rounds, a.batch))
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
