"""The training objective of the monocular main loop (train.py:300-456), torch form against the fused HIP form (dynibar_amd.objective).
GPU only -- there is no CPU path.

  python tools/objectivebench.py [--seconds 1.0] [--rounds 5]   # one JSON line: both forms at 3072 x 64 (10 dynamic views: T = 7 trajectory
        # frames, 6 flow views) and at 1024 x 128, and inside a whole training iteration (tools/train_case.py)
  python tools/objectivebench.py --rocprof profiles/objective_kernel_stats.txt
        # the same loops in a child process under rocprofv3 --kernel-trace --stats, summarised by tools/rocpd_summary.py

(a) the torch form: the loss written with dynibar_amd.criterion and plain torch exactly as train.py has it (torch_form below), its autograd
backward and the seven .item() calls of scalars_to_log -- what a user of the package ran before dynibar_amd.objective existed;
(b) MonoObjective: forward + backward + ONE copy of the logged scalars to the host.
Both are timed alternating in the same process after warm-up, device-synchronised, in rounds of at least --seconds each; the spread over the
rounds is reported next to the median.  Peak memory is torch's allocator peak above the inputs.  The whole-iteration pair runs
render_rays_mono(is_train=True) + objective + backward at the kid-running shape.  bench.py's training figure uses neither: its loss is a dot
product with fixed cotangents.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

KID = dict(w_disp=0.1, w_flow=0.01, w_cycle=0.1, w_reg=0.05, w_skew_entropy=5e-4, w_distortion=1e-3, decay_rate=10, init_decay_epoch=400,
           anneal_cycle=True, cycle_factor=0.1)  # configs/train_kid-running.txt
LOG7 = ('loss', 'flow', 'disp', 'cycle', 'reg', 'entropy', 'static')  # (train.py:454-466 logs seven of them)


def distloss_torch(w, m, interval):
  """the published O(N) form of torch_efficient_distloss.eff_distloss_native in torch ops (the package is a dependency this repository does not have)"""
  import torch
  loss_uni = (1.0 / 3.0) * (interval * w.pow(2)).sum(dim=-1).mean()
  wm = w * m
  w_cs, wm_cs = w.cumsum(dim=-1), wm.cumsum(dim=-1)
  return 2.0 * (wm[..., 1:] * w_cs[..., :-1] - w[..., 1:] * wm_cs[..., :-1]).sum(dim=-1).mean() + loss_uni


def torch_form(ret, ray_batch, epoch, args):
  """train.py:300-456 as the script has it, on dynibar_amd.criterion -> (loss, scalars_to_log); seven .item() synchronisations"""
  import torch
  from dynibar_amd.criterion import Criterion, compute_flow_loss, compute_rgb_loss, compute_temporal_rgb_loss
  rgb_criterion = Criterion()
  decay_rate = args.decay_rate
  divisor = epoch // args.init_decay_epoch
  rgb_loss = rgb_criterion(ret['outputs_coarse_ref'], ray_batch)
  rgb_loss += compute_temporal_rgb_loss(ret['outputs_coarse_anchor'], ray_batch)
  if epoch < args.init_decay_epoch:
    dynamic_mask = ret['outputs_coarse_ref']['mask'].float() * ray_batch['motion_mask'].float()
    rgb_loss += compute_rgb_loss(ret['outputs_coarse_ref']['rgb_dy'], ray_batch, dynamic_mask)
  rgb_loss += rgb_criterion(ret['outputs_coarse_ref_dy'], ray_batch, motion_mask=ray_batch['motion_mask'].float()) / (10.0 ** divisor)
  rgb_loss += compute_temporal_rgb_loss(ret['outputs_coarse_anchor_dy'], ray_batch, motion_mask=ray_batch['motion_mask'].float()) / (10.0 ** divisor)
  w_disp = args.w_disp / (decay_rate ** divisor)
  pred_disp = 1.0 / torch.clamp(ret['outputs_coarse_ref']['depth'], min=1e-2)
  pred_mask = ret['outputs_coarse_ref']['mask']
  disp_loss = w_disp * torch.sum(torch.abs(pred_disp - ray_batch['disp']) * pred_mask) / (torch.sum(pred_mask) + 1e-8)
  w_flow = args.w_flow / (decay_rate ** divisor)
  nv = ret['outputs_coarse_ref']['render_flows'].shape[0]
  flow_mask = pred_mask[None, :, None] * ray_batch['masks'][:nv]
  flow_loss = w_flow * compute_flow_loss(ret['outputs_coarse_ref']['render_flows'], ray_batch['flows'][:nv], flow_mask)
  w_cycle = min(0.5, args.w_cycle + divisor * args.cycle_factor) if args.anneal_cycle else args.w_cycle
  pts_traj_anchor = ret['outputs_coarse_anchor']['pts_traj_anchor']
  pts_traj_ref = ret['outputs_coarse_anchor']['pts_traj_ref']
  occ_weights = ret['outputs_coarse_anchor']['occ_weights'][None, ..., None].repeat(pts_traj_anchor.shape[0], 1, 1, pts_traj_anchor.shape[-1])
  cycle_loss = w_cycle * torch.sum(torch.abs(pts_traj_ref - pts_traj_anchor) * occ_weights) / (torch.sum(occ_weights) + 1e-8)
  sf = ret['outputs_coarse_anchor']['sf_seq']
  reg_loss = args.w_reg * torch.mean(torch.abs(sf))
  reg_loss += args.w_reg * 0.5 * torch.mean(torch.pow(sf[:-1] - sf[1:], 2))
  reg_loss += args.w_reg * torch.mean(torch.abs(sf[:, :, 1:, :] - sf[:, :, :-1, :]))
  render_weights_dy = torch.sum(ret['outputs_coarse_ref']['weights_dy'], dim=-1)
  render_weights_st = torch.sum(ret['outputs_coarse_ref']['weights_st'], dim=-1)
  weights_ratio = render_weights_dy / torch.clamp(render_weights_dy + render_weights_st, min=1e-9)
  entropy_loss = -(weights_ratio * torch.log(weights_ratio + 1e-9) + (1.0 - weights_ratio) * torch.log(1.0 - weights_ratio + 1e-9))
  entropy_loss = args.w_skew_entropy * torch.mean(entropy_loss)
  s_vals = ret['outputs_coarse_ref']['s_vals']
  mid_dist = (s_vals[:, 1:] + s_vals[:, :-1]) * 0.5
  interval = s_vals[:, 1:] - s_vals[:, :-1]
  distortion_loss = args.w_distortion * distloss_torch(ret['outputs_coarse_ref']['weights'][:, :-1], mid_dist, interval)
  static_static_mask = 1.0 - ray_batch['static_mask'].float()
  static_static_mask *= ret['outputs_coarse_ref']['mask'].float()
  static_static_mask *= (1.0 - weights_ratio).float().detach()
  static_loss = compute_rgb_loss(ret['outputs_coarse_ref']['rgb_static'], ray_batch, static_static_mask)
  if divisor > 4:
    static_sfm_mask_2 = static_static_mask * (weights_ratio < 0.1).float()
    static_loss += 0.1 * torch.sum(torch.abs(render_weights_dy * static_sfm_mask_2.detach())) / torch.sum(static_sfm_mask_2 + 1e-8)
  loss = rgb_loss + cycle_loss + flow_loss + disp_loss + reg_loss + entropy_loss + distortion_loss + static_loss
  return loss, dict(loss=loss, flow=flow_loss, disp=disp_loss, cycle=cycle_loss, reg=reg_loss, entropy=entropy_loss, static=static_loss)


def seeded_case(R, S, T, nv, dev):
  """a ret-shaped dictionary and targets on the device (seeded; the leaves require grad)"""
  import torch
  g = torch.Generator().manual_seed(7)
  r = lambda *s: torch.rand(*s, generator=g)
  n = lambda *s: torch.randn(*s, generator=g)
  rows = lambda: (lambda x: x / x.sum(-1, keepdim=True))(r(R, S) ** 3 + 1e-6)
  rho, tot = r(R, 1), 0.3 + 0.6 * r(R, 1)
  L = lambda x: x.to(dev).requires_grad_(True)
  C = lambda x: x.to(dev)
  nt = int(round(0.1 * S))
  pr, pa, sf = n(T, R, S, 3), n(T, R, S, 3), 0.1 * n(6, R, S, 3)
  pa[:, :, S - nt:] = pr[:, :, S - nt:]
  sf[:, :, S - nt:] = 0.0
  ref = dict(rgb=L(r(R, 3)), rgb_dy=L(r(R, 3)), rgb_static=L(r(R, 3)), depth=L(0.005 + 3.0 * r(R)), render_flows=L(4.0 * n(nv, R, 2)),
             weights=L(rows() * 0.9), weights_dy=L(rows() * rho * tot), weights_st=L(rows() * (1.0 - rho) * tot),
             s_vals=C(torch.sort(r(R, S), dim=-1).values), mask=C(r(R) < 0.9))
  anc = dict(rgb=L(r(R, 3)), mask=C(r(R) < 0.9), occ_weight_map=C(r(R)), occ_weights=C(1.0 - 0.5 * r(R, S)), pts_traj_ref=L(pr), pts_traj_anchor=L(pa),
             sf_seq=L(sf))
  ret = dict(outputs_coarse_ref=ref, outputs_coarse_anchor=anc, outputs_coarse_ref_dy=dict(rgb=L(r(R, 3)), mask=C(r(R) < 0.9)),
             outputs_coarse_anchor_dy=dict(rgb=L(r(R, 3)), mask=C(r(R) < 0.9), occ_weight_map=C(r(R))))
  batch = dict(rgb=C(r(R, 3)), disp=C(0.05 + 0.5 * r(R)), flows=C(4.0 * n(nv, R, 2)), masks=C((r(nv, R, 1) < 0.8).float()),
               motion_mask=C((r(R) < 0.5).float()), static_mask=C((r(R) < 0.3).float()))
  leaves = [v for d in ret.values() for v in d.values() if v.requires_grad]
  return ret, batch, leaves


def _stats(xs):
  xs = sorted(xs)
  return dict(median_ms=round(xs[len(xs) // 2], 4), min_ms=round(xs[0], 4), max_ms=round(xs[-1], 4))


def alternate(fa, fb, seconds, rounds, warmup=5):
  """time fa and fb alternating: per round each runs for at least `seconds`, synchronised at both ends -> per-call ms of every round"""
  import torch
  for _ in range(warmup):
    fa()
    fb()
  torch.cuda.synchronize()
  out = ([], [])
  for _ in range(rounds):
    for f, dst in ((fa, out[0]), (fb, out[1])):
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


def peak_mb(f):
  import torch
  f()
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  f()
  torch.cuda.synchronize()
  return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def run(seconds, rounds, iteration=True, epoch=0):
  import torch
  from dynibar_amd import _lib, objective
  assert torch.cuda.is_available(), 'objectivebench needs an MI355X (there is no CPU path)'
  _lib.lib()
  dev = torch.device('cuda:0')
  args = types.SimpleNamespace(**KID)
  obj = objective.MonoObjective(args)
  out = {'metric': 'objective_ms', 'epoch': epoch, 'seconds_per_round': seconds, 'rounds': rounds, 'shapes': {}}
  for R, S in ((3072, 64), (1024, 128)):
    ret, batch, leaves = seeded_case(R, S, 7, 6, dev)

    def zero():
      for v in leaves:
        v.grad = None

    def torch_step():
      zero()
      loss, log = torch_form(ret, batch, epoch, args)
      loss.backward()
      return {k: v.item() for k, v in log.items()}

    def fused_step():
      zero()
      loss, logged = obj(ret, batch, epoch)
      loss.backward()
      return dict(zip(objective.LOGGED, logged.tolist()))

    a, b = torch_step(), fused_step()
    assert abs(a['loss'] - b['loss']) <= 1e-5 + 2e-4 * abs(a['loss']), (a, b)
    ta, tb = alternate(torch_step, fused_step, seconds, rounds)
    out['shapes'][f'{R}x{S}'] = dict(torch=_stats(ta), fused=_stats(tb), speedup_median=round(_stats(ta)['median_ms'] / _stats(tb)['median_ms'], 2),
                                     torch_peak_mb=peak_mb(torch_step), fused_peak_mb=peak_mb(fused_step), loss_torch=a['loss'], loss_fused=b['loss'],
                                     host_copies_torch=len(LOG7), host_copies_fused=1)
    del ret, batch, leaves
  if iteration:
    from train_case import TrainCase
    tc = TrainCase('cuda:0')
    g = torch.Generator().manual_seed(5)
    R = tc.R
    batch = dict(rgb=torch.rand(R, 3, generator=g), disp=0.05 + 0.5 * torch.rand(R, generator=g), flows=4.0 * torch.randn(6, R, 2, generator=g),
                 masks=(torch.rand(6, R, 1, generator=g) < 0.8).float(), motion_mask=(torch.rand(R, generator=g) < 0.5).float(),
                 static_mask=(torch.rand(R, generator=g) < 0.3).float())
    batch = {k: v.to(dev) for k, v in batch.items()}
    from dynibar_amd import render_ray

    def render():
      for p in tc.parameters():
        p.grad = None
      return render_ray.render_rays_mono(tc.fidx, tc.temb, tc.toff, tc.batch, tc.model, tc.feat, tc.proj, tc.S, tc.args, inv_uniform=True, det=True,
                                         is_train=True, num_vv=tc.num_vv)

    def it_torch():
      loss, log = torch_form(render(), batch, epoch, args)
      loss.backward()
      return {k: v.item() for k, v in log.items()}

    def it_fused():
      loss, logged = obj(render(), batch, epoch)
      loss.backward()
      return logged.tolist()

    ta, tb = alternate(it_torch, it_fused, seconds, rounds, warmup=2)
    out['iteration_3072x64'] = dict(torch=_stats(ta), fused=_stats(tb), torch_peak_mb=peak_mb(it_torch), fused_peak_mb=peak_mb(it_fused))
  return out


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--seconds', type=float, default=1.0)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--no-iteration', action='store_true')
  ap.add_argument('--rocprof', default=None, help='write the rocprofv3 kernel stats of a separate run to this file')
  ap.add_argument('--only', choices=('torch', 'fused'), default=None, help='(internal: the child runs under the profiler) 20 steps of one form at 3072 x 64')
  a = ap.parse_args()
  if a.only:
    import torch
    from dynibar_amd import objective
    args = types.SimpleNamespace(**KID)
    ret, batch, leaves = seeded_case(3072, 64, 7, 6, torch.device('cuda:0'))
    obj = objective.MonoObjective(args)
    for _ in range(20):
      for v in leaves:
        v.grad = None
      if a.only == 'torch':
        loss, log = torch_form(ret, batch, 0, args)
        loss.backward()
        _ = {k: v.item() for k, v in log.items()}
      else:
        loss, logged = obj(ret, batch, 0)
        loss.backward()
        _ = logged.tolist()
    torch.cuda.synchronize()
    return
  if a.rocprof:
    import glob
    import tempfile
    parts = []
    for form in ('torch', 'fused'):
      d = tempfile.mkdtemp(prefix=f'objectivebench_{form}_')
      cmd = ['timeout', '-k', '10', '300', 'rocprofv3', '--kernel-trace', '--stats', '-d', d, '--', sys.executable, os.path.abspath(__file__), '--only', form]
      subprocess.run(cmd, check=True, cwd=d)  # (a failure ends the tool: nothing more is started on the GPU)
      dbs = sorted(glob.glob(os.path.join(d, '**', '*.db'), recursive=True))
      assert dbs, f'rocprofv3 wrote no database under {d}'
      txt = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rocpd_summary.py'), 'stats', dbs[0]], check=True, capture_output=True,
                           text=True).stdout.replace(d, '<run dir>')
      calls = sum(int(l.split()[-13]) for l in txt.splitlines()[2:] if l.strip())
      parts.append(f'## {form} form: python tools/objectivebench.py --only {form}  (20 steps of forward + backward + logging at 3072 x 64, T = 7, 6 flow '
                   f'views; {calls} kernel launches = {calls / 20:.1f} per step)\n{txt}')
    os.makedirs(os.path.dirname(os.path.abspath(a.rocprof)), exist_ok=True)
    with open(a.rocprof, 'w') as f:
      f.write('\n'.join(parts))
    print('\n'.join(parts))
    return
  print(json.dumps(run(a.seconds, a.rounds, not a.no_iteration)))


if __name__ == '__main__':
  main()
