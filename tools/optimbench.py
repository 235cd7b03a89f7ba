"""The optimizer step on the kid-running model's parameter set: dynibar_amd.optim.Adam (one k_adam_step launch) against torch.optim.Adam, in one
process on the same gradients.  GPU only -- there is no CPU path.

  python tools/optimbench.py [--rounds 30] [--inner 20] [--out profiles/optimizer.txt] [--weight-decay L] [--adamw] [--amsgrad] [--maximize] [--capturable]

The parameter set is the model's (ibrnet/model.py:341-364): the static and the dynamic MLP, the motion MLP (shapes of dynibar_amd.synthetic's layer
tables), the two ResNet encoders (its encoder weights) and the trajectory basis, in the reference's six groups with its four learning rates
(configs/train_kid-running.txt: lrate_mlp 4e-4, lrate_feature 8e-4), with seeded random gradients.  One step of this optimizer is first compared
with the numpy restatement of the contract (tests/optim_cases.py), exactly.  Then four legs alternate after a warm-up, each on its own copy of the
parameters: (1) this optimizer, (2) torch.optim.Adam with its default implementation, (3) the same again -- the spread between two identical
legs --, (4) torch.optim.Adam(foreach=False), the per-tensor loop the reference's torch ran.  A leg is `inner` steps timed by the host clock
around work that ends in a stream synchronise.  In a separate pass the kernel's own time comes from the library's events, and with it the
bytes the kernel moves (16 read and 12 written per element) over that time.  The loop leaves the ~30 MB working set in the 256 MiB Infinity
Cache between steps; in training the rest of the iteration passes through the cache in between.  No ratio is fixed in advance.
The guard (step(max_grad_norm=..., skip_nonfinite=True): k_grad_sumsq, k_grad_stats, k_adam_step_guarded) is timed in a pass of its own after those,
so the four legs above keep their layout: the guarded step twice (the spread of two identical legs), torch.nn.utils.clip_grad_norm_ followed by
torch.optim.Adam.step() on the same gradients, and optim.grad_norm alone.  The legs share their gradient tensors, so max_norm is far above the norm:
coef is 1, torch multiplies every gradient by 1.0 (its cost is the same, the gradients stay), the guarded kernel multiplies by 1 as it always does.
One guarded step is first compared with the restatement of tests/optim_guard_cases.py, exactly; the three kernels' own times come from the events.
With one of the option flags the extended step (k_adamx_step, k_adam_advance) gets a further pass of its own: one step with the options against
the restatement of tests/optim_ext_cases.py, exactly, then the plain step twice (its spread), the step with the options, the extended kernel
with no option set, torch's optimizer with the same options and the guarded step with the options; the ratios are reported, none is asserted."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

LRATE_MLP, LRATE_FEATURE = 4e-4, 8e-4


def parameter_set():
  """[(lr, [numpy float32 arrays])]: the six groups of model.py:341-364 in its order"""
  import numpy as np
  from dynibar_amd import synthetic as syn
  import train_case
  basis = np.random.default_rng(5).standard_normal((train_case.NUM_FRAMES, train_case.NUM_BASIS)).astype(np.float32)
  return [(LRATE_MLP * 0.5, list(syn.make_weights('static', 0).values())),
          (LRATE_FEATURE * 0.5, list(syn.make_encoder_weights(1).values())),
          (LRATE_MLP, list(syn.make_weights('dynamic', 0).values())),
          (LRATE_FEATURE, list(syn.make_encoder_weights(0).values())),
          (LRATE_MLP, list(syn.make_weights('motion', 0, num_basis=train_case.NUM_BASIS).values())),
          (LRATE_MLP * 0.25, [basis])]


def run(rounds, inner, dev='cuda:0', options=None):
  import numpy as np
  import torch
  import optim_cases as oc
  from dynibar_amd import _lib, optim
  groups = parameter_set()
  rng = np.random.default_rng(31)
  host_grads = [[oc.gradient(rng, a.size).reshape(a.shape) for a in arrs] for _, arrs in groups]
  grads = [[torch.from_numpy(g).to(dev) for g in gs] for gs in host_grads]

  def make(cls, **kw):
    ps = [[torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in arrs] for _, arrs in groups]
    for pg, gg in zip(ps, grads):
      for p, g in zip(pg, gg):
        p.grad = g
    return ps, cls([{'params': pg if i < 5 else pg[0], 'lr': lr} for i, ((lr, _), pg) in enumerate(zip(groups, ps))], **kw)

  # one step against the restatement, exactly
  ps, opt = make(optim.Adam)
  opt.step()
  torch.cuda.synchronize()
  for (lr, arrs), pg, gs in zip(groups, ps, host_grads):
    for a, p, g in zip(arrs, pg, gs):
      n = a.size
      wp, wm, wv = oc.restate(a.reshape(-1), g.reshape(-1), np.zeros(n, np.float32), np.zeros(n, np.float32), lr, 0.9, 0.999, 1e-8, 1)
      oc.same(wp, p, 'p')
      oc.same(wm, opt.state[p]['exp_avg'], 'm')
      oc.same(wv, opt.state[p]['exp_avg_sq'], 'v')

  legs = [('hip', make(optim.Adam)[1]), ('torch_default', make(torch.optim.Adam)[1]), ('torch_default_again', make(torch.optim.Adam)[1]),
          ('torch_foreach_false', make(torch.optim.Adam, foreach=False)[1])]
  times = {name: [] for name, _ in legs}
  for r in range(rounds + 2):
    for name, o in legs:
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(inner):
        o.step()
      torch.cuda.synchronize()
      if r >= 2:
        times[name].append((time.perf_counter() - t0) * 1e3 / inner)
  # the fused clearing against step + zero_grad(set_to_none=False), each on gradients of its own
  pz, oz = make(optim.Adam)
  for pg in pz:
    for p in pg:
      p.grad = p.grad.clone()
  clear = {'hip_step_zero_grads': [], 'hip_step_then_zero_grad': []}
  for r in range(rounds + 2):
    for name in clear:
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(inner):
        if name == 'hip_step_zero_grads':
          oz.step(zero_grads=True)
          oz.zero_grad(set_to_none=False)
        else:
          oz.step()
          oz.zero_grad(set_to_none=False)
      torch.cuda.synchronize()
      if r >= 2:
        clear[name].append((time.perf_counter() - t0) * 1e3 / inner)
  # the guard, in a pass of its own
  import optim_guard_cases as gc
  ps, opt = make(optim.Adam)
  flat = [g.reshape(-1) for gs in host_grads for g in gs]
  partials, st = gc.restate_norm(flat, optim.CHUNK, 1.0)
  opt.step(max_grad_norm=1.0, skip_nonfinite=True)
  torch.cuda.synchronize()
  gc.same64(partials, opt._tables['partials'], 'partials')
  oc.same(np.array([st['norm']]), opt.grad_stats.norm, 'norm')
  oc.same(np.array([st['coef']]), opt.grad_stats.coef, 'coef')
  assert st['coef'] < 1 and int(opt.grad_stats.finite) == 1
  for (lr, arrs), pg, gs in zip(groups, ps, host_grads):
    for a, p, g in zip(arrs, pg, gs):
      n = a.size
      wp, wm, wv = oc.restate(a.reshape(-1), gc.scaled(g.reshape(-1), st['coef']), np.zeros(n, np.float32), np.zeros(n, np.float32), lr, 0.9, 0.999,
                              1e-8, 1)
      oc.same(wp, p, 'guarded p')
      oc.same(wm, opt.state[p]['exp_avg'], 'guarded m')
      oc.same(wv, opt.state[p]['exp_avg_sq'], 'guarded v')
  FAR = 1e30
  tps, topt = make(torch.optim.Adam)
  tflat = [p for pg in tps for p in pg]

  def torch_clip_step():
    torch.nn.utils.clip_grad_norm_(tflat, FAR)
    topt.step()

  guarded = [make(optim.Adam)[1] for _ in range(2)]
  guard_legs = [('hip_guarded', lambda: guarded[0].step(max_grad_norm=FAR, skip_nonfinite=True)), ('torch_clip_then_step', torch_clip_step),
                ('hip_guarded_again', lambda: guarded[1].step(max_grad_norm=FAR, skip_nonfinite=True)),
                ('hip_unguarded', legs[0][1].step), ('hip_grad_norm_alone', lambda: optim.grad_norm(tflat))]
  gtimes = {name: [] for name, _ in guard_legs}
  for r in range(rounds + 2):
    for name, fn in guard_legs:
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(inner):
        fn()
      torch.cuda.synchronize()
      if r >= 2:
        gtimes[name].append((time.perf_counter() - t0) * 1e3 / inner)
  # the kernel's own time
  lib = _lib.lib()
  nk = lib.dyn_profile_count()
  ms, cnt = np.zeros(nk, np.float32), np.zeros(nk, np.int32)
  hip = legs[0][1]
  lib.dyn_profile_enable(1)
  lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
  for _ in range(rounds * inner):
    hip.step()
  torch.cuda.synchronize()
  lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
  lib.dyn_profile_enable(0)
  kern = {lib.dyn_profile_name(i).decode(): (float(ms[i]) / int(cnt[i]), int(cnt[i])) for i in range(nk) if cnt[i]}
  assert list(kern) == ['k_adam_step'] and kern['k_adam_step'][1] == rounds * inner, kern
  kernel_ms = kern['k_adam_step'][0]
  lib.dyn_profile_enable(1)
  lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
  for _ in range(rounds * inner):
    guarded[0].step(max_grad_norm=FAR, skip_nonfinite=True)
  torch.cuda.synchronize()
  lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
  lib.dyn_profile_enable(0)
  gkern = {lib.dyn_profile_name(i).decode(): (float(ms[i]) / int(cnt[i]), int(cnt[i])) for i in range(nk) if cnt[i]}
  assert sorted(gkern) == ['k_adam_step_guarded', 'k_grad_stats', 'k_grad_sumsq'] and all(c == rounds * inner for _, c in gkern.values()), gkern
  elements = sum(a.size for _, arrs in groups for a in arrs)
  tensors = sum(len(arrs) for _, arrs in groups)
  extended = None
  if options is not None:  # the extended step with the options of the command line, in a pass of its own
    import optim_ext_cases as xc
    okw = {k: v for k, v in options.items() if k != 'adamw'}
    ours_cls, torch_cls = (optim.AdamW, torch.optim.AdamW) if options['adamw'] else (optim.AdamX, torch.optim.Adam)
    lam, dec = okw.get('weight_decay', 1e-2 if options['adamw'] else 0.0), options['adamw']
    ps, opt = make(ours_cls, **okw)
    opt.step()
    torch.cuda.synchronize()
    for (lr, arrs), pg, gs in zip(groups, ps, host_grads):  # one step against the restatement, exactly
      for a, p, g in zip(arrs, pg, gs):
        n = a.size
        a1, s21 = xc.pow_scalars(lr, 0.9, 0.999, np.ones(2))[:2] if okw.get('capturable') else oc.scalars(lr, 0.9, 0.999, 1)
        wp, wm, wv, wx = xc.restate(a.reshape(-1), g.reshape(-1), np.zeros(n, np.float32), np.zeros(n, np.float32),
                                    np.zeros(n, np.float32) if okw.get('amsgrad') else None, a1, s21, 0.9, 0.999, 1e-8, wd=0.0 if dec else lam,
                                    decay=xc.decay_factor(lr, lam) if dec and lam else 1.0, maximize=bool(okw.get('maximize')))
        oc.same(wp, p, 'extended p')
        oc.same(wm, opt.state[p]['exp_avg'], 'extended m')
        oc.same(wv, opt.state[p]['exp_avg_sq'], 'extended v')
        if wx is not None:
          oc.same(wx, opt.state[p]['max_exp_avg_sq'], 'extended vmax')
    forced = make(optim.AdamX)[1]
    forced.extended_kernel = True  # the extended kernel with no option set: what its record and its branches cost on their own
    xlegs = [('hip_plain', legs[0][1].step), ('hip_options', opt.step), ('hip_plain_again', make(optim.Adam)[1].step),
             ('hip_extended_kernel_no_options', forced.step), ('torch_options', make(torch_cls, **okw)[1].step),
             ('hip_options_guarded', lambda o=make(ours_cls, **okw)[1]: o.step(max_grad_norm=1e30, skip_nonfinite=True))]
    xtimes = {name: [] for name, _ in xlegs}
    for r in range(rounds + 2):
      for name, fn in xlegs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
          fn()
        torch.cuda.synchronize()
        if r >= 2:
          xtimes[name].append((time.perf_counter() - t0) * 1e3 / inner)
    xkern = {}
    for tag, o in (('options', opt), ('no_options', forced)):
      lib.dyn_profile_enable(1)
      lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
      for _ in range(rounds * inner):
        o.step()
      torch.cuda.synchronize()
      lib.dyn_profile_read(ms.ctypes.data, cnt.ctypes.data)
      lib.dyn_profile_enable(0)
      xkern[tag] = {lib.dyn_profile_name(i).decode(): round(float(ms[i]) / int(cnt[i]), 5) for i in range(nk) if cnt[i]}
      assert 'k_adamx_step' in xkern[tag] and 'k_adam_step' not in xkern[tag], xkern
    xmed = {name: statistics.median(v) for name, v in xtimes.items()}
    per = 28 + (8 if okw.get('amsgrad') else 0)
    q = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    extended = dict(options=options, step_ms={name: q(v) for name, v in xtimes.items()}, kernel_ms=xkern, bytes_per_element=per,
                    plain_spread_ms=round(abs(xmed['hip_plain'] - xmed['hip_plain_again']), 4),
                    options_over_plain=round(xmed['hip_options'] / min(xmed['hip_plain'], xmed['hip_plain_again']), 4),
                    kernel_options_over_plain=round(xkern['options']['k_adamx_step'] / kernel_ms, 4),
                    kernel_tb_per_s=round(per * elements / (xkern['options']['k_adamx_step'] * 1e-3) / 1e12, 3), exact=True)
  moved = 28 * elements
  q = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
  res = {name: q(v) for name, v in times.items()}
  med = {name: statistics.median(v) for name, v in times.items()}
  spread = abs(med['torch_default'] - med['torch_default_again'])
  gmed = {name: statistics.median(v) for name, v in gtimes.items()}
  guard = dict(step_ms={name: q(v) for name, v in gtimes.items()}, max_norm=FAR,
               guarded_spread_ms=round(abs(gmed['hip_guarded'] - gmed['hip_guarded_again']), 4),
               guarded_minus_unguarded_ms=round(min(gmed['hip_guarded'], gmed['hip_guarded_again']) - gmed['hip_unguarded'], 4),
               guarded_minus_torch_clip_then_step_ms=round(min(gmed['hip_guarded'], gmed['hip_guarded_again']) - gmed['torch_clip_then_step'], 4),
               kernel_ms={k: round(v[0], 5) for k, v in sorted(gkern.items())}, kernels_ms=round(sum(v[0] for v in gkern.values()), 5),
               sumsq_tb_per_s=round(4 * elements / (gkern['k_grad_sumsq'][0] * 1e-3) / 1e12, 3))
  return dict(tensors=tensors, elements=elements, groups=len(groups), chunks=hip._tables['n_chunks'], chunk=optim.CHUNK, rounds=rounds, inner=inner,
              step_ms=res, clearing_ms={k: q(v) for k, v in clear.items()}, torch_default_spread_ms=round(spread, 4),
              hip_minus_torch_default_ms=round(med['hip'] - min(med['torch_default'], med['torch_default_again']), 4),
              hip_no_slower_than_torch_default=bool(med['hip'] <= max(med['torch_default'], med['torch_default_again']) + spread),
              kernel_ms=round(kernel_ms, 5), kernel_bytes=moved, kernel_tb_per_s=round(moved / (kernel_ms * 1e-3) / 1e12, 3),
              share_of_8_tb_per_s=round(moved / (kernel_ms * 1e-3) / 8e12, 3), exact=True, guard=guard, extended=extended, device=torch.cuda.get_device_name(0), torch=torch.__version__)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=30)
  ap.add_argument('--inner', type=int, default=20)
  ap.add_argument('--out', default=None)
  ap.add_argument('--weight-decay', type=float, default=None, help='the extended step: coupled weight decay (decoupled with --adamw)')
  ap.add_argument('--adamw', action='store_true', help='the extended step: optim.AdamW against torch.optim.AdamW (weight decay 1e-2 unless given)')
  ap.add_argument('--amsgrad', action='store_true')
  ap.add_argument('--maximize', action='store_true')
  ap.add_argument('--capturable', action='store_true', help='step counts on the device (k_adam_advance follows the step)')
  a = ap.parse_args()
  options = None
  if a.weight_decay is not None or a.adamw or a.amsgrad or a.maximize or a.capturable:
    options = dict(adamw=a.adamw, amsgrad=a.amsgrad, maximize=a.maximize, capturable=a.capturable)
    if a.weight_decay is not None:
      options['weight_decay'] = a.weight_decay
  line = json.dumps(run(a.rounds, a.inner, options=options))
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
