"""Support for the objective tests (dynibar_amd/objective.py): a seeded generator of the dictionary render_rays_mono(is_train=True) returns
plus the data loader's supervision, a plain-torch restatement of the reference's main-loop loss WITH its schedule (train.py:300-456;
cases.mono_train_loss has no anneal_cycle and no divisor > 4 branch), and the one helper the emulator and the device tests share.
Test infrastructure: nothing in dynibar_amd imports this."""
import types

import torch

import cases
import parity

# configs/train_kid-running.txt (the weights the gradient goldens were made with: cases.mono_train_loss's docstring)
KID_ARGS = dict(w_disp=0.1, w_flow=0.01, w_cycle=0.1, w_reg=0.05, w_skew_entropy=5e-4, w_distortion=1e-3, decay_rate=10, init_decay_epoch=400,
                anneal_cycle=True, cycle_factor=0.1)
ALL = ('rgb', 'disp', 'flow', 'cycle', 'reg', 'entropy', 'distortion', 'static')
LOGGED = ('loss', 'rgb', 'cycle', 'flow', 'disp', 'reg', 'entropy', 'distortion', 'static')
# (group, key) of every tensor of `ret` the loss differentiates
LEAVES = (('outputs_coarse_ref', 'rgb'), ('outputs_coarse_ref', 'rgb_dy'), ('outputs_coarse_ref', 'rgb_static'), ('outputs_coarse_ref', 'depth'),
          ('outputs_coarse_ref', 'render_flows'), ('outputs_coarse_ref', 'weights'), ('outputs_coarse_ref', 'weights_dy'),
          ('outputs_coarse_ref', 'weights_st'), ('outputs_coarse_ref_dy', 'rgb'), ('outputs_coarse_anchor', 'rgb'),
          ('outputs_coarse_anchor_dy', 'rgb'), ('outputs_coarse_anchor', 'pts_traj_ref'), ('outputs_coarse_anchor', 'pts_traj_anchor'),
          ('outputs_coarse_anchor', 'sf_seq'))
# the epochs that take every branch of the schedule with init_decay_epoch = 400: divisor 0, 1 (the dynamic-only colour term gone, the decays on),
# 5 (divisor > 4: the static addition; anneal_cycle at its 0.5 cap: 0.1 + 5 * 0.1 = 0.6)
EPOCHS = (0, 400, 2000)


def args_of(**over):
  return types.SimpleNamespace(**{**KID_ARGS, **over})


def n_tail(S):
  return int(round(S * 0.1))  # render_ray.py: the motion coefficients of a ray's last samples are zeroed


def make_case(R, S, nv=6, T=4, seed=7):
  """Seeded fp32 stand-ins for ret / ray_batch (CPU).  weights_dy / weights_st: normalised rand**3 rows scaled per ray so that the ratio is
  spread over 0..1; depth = 0.005 + 3 rand (a few rays below the 1e-2 clamp); masks at 0.9; randn trajectories; sf_seq and
  pts_traj_ref - pts_traj_anchor exactly 0 on each ray's last round(0.1 S) samples, as the renderer leaves them.  Threshold ties are removed at
  the source: a ray whose float64 ratio lies within 1e-4 of 0.1 gets weights_dy scaled by 1.01."""
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32)
  n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
  rows = lambda: (lambda x: x / x.sum(-1, keepdim=True))(r(R, S) ** 3 + 1e-6)
  rho, tot = r(R, 1), 0.3 + 0.6 * r(R, 1)
  wdy, wst = rows() * rho * tot, rows() * (1.0 - rho) * tot
  for _ in range(3):
    a, b = wdy.double().sum(-1), wst.double().sum(-1)
    tie = ((a / (a + b).clamp(min=1e-9)) - 0.1).abs() < 1e-4
    wdy = torch.where(tie[:, None], wdy * 1.01, wdy)
  s_vals = torch.sort(r(R, S), dim=-1).values
  mask = lambda: r(R) < 0.9
  nt = n_tail(S)
  pr, pa, sf = n(T, R, S, 3), n(T, R, S, 3), 0.1 * n(6, R, S, 3)
  if nt > 0:
    pa[:, :, S - nt:] = pr[:, :, S - nt:]
    sf[:, :, S - nt:] = 0.0
  ref = dict(rgb=r(R, 3), rgb_dy=r(R, 3), rgb_static=r(R, 3), depth=0.005 + 3.0 * r(R), render_flows=4.0 * n(nv, R, 2), weights=rows() * 0.9,
             weights_dy=wdy, weights_st=wst, s_vals=s_vals, mask=mask())
  anc = dict(rgb=r(R, 3), mask=mask(), occ_weight_map=r(R), occ_weights=1.0 - 0.5 * r(R, S), pts_traj_ref=pr, pts_traj_anchor=pa, sf_seq=sf)
  ret = dict(outputs_coarse_ref=ref, outputs_coarse_anchor=anc, outputs_coarse_ref_dy=dict(rgb=r(R, 3), mask=mask()),
             outputs_coarse_anchor_dy=dict(rgb=r(R, 3), mask=mask(), occ_weight_map=r(R)))
  tgt = cases.train_batch_targets(R, n_flow_views=max(nv, 1), seed=seed + 100)
  return ret, tgt


def assert_no_ties(ret):
  ref = ret['outputs_coarse_ref']
  a, b = ref['weights_dy'].double().sum(-1), ref['weights_st'].double().sum(-1)
  ratio = a / (a + b).clamp(min=1e-9)
  assert int(((ratio - 0.1).abs() < 1e-4).sum()) == 0, 'a weights ratio within 1e-4 of the 0.1 threshold'
  assert int(((ref['depth'].double() - 1e-2).abs() < 1e-6).sum()) == 0, 'a depth within 1e-6 of the 1e-2 clamp'
  return ratio


def instantiate(ret, tgt, dtype, device, trainable=None):
  """copies of the case in `dtype` on `device`; the LEAVES in `trainable` (None: all) require grad -> (ret, tgt, {leaf: tensor})"""
  out, leaves = {}, {}
  for grp, d in ret.items():
    out[grp] = {}
    for k, v in d.items():
      v = (v.to(dtype) if v.is_floating_point() else v).to(device).clone()
      if (grp, k) in LEAVES and (trainable is None or (grp, k) in trainable):
        v.requires_grad_(True)
        leaves[(grp, k)] = v
      out[grp][k] = v
  return out, {k: (v.to(dtype) if v.is_floating_point() else v).to(device) for k, v in tgt.items()}, leaves


def charb(x, y, mask):
  """utils.img2charbonier (utils.py:32-39), EPSILON = 0.001 (criterion.py:19), TINY_NUMBER = 1e-6"""
  return torch.sum(torch.sqrt((x - y) ** 2 + 0.001 ** 2) * mask.unsqueeze(-1)) / (torch.sum(mask) * x.shape[-1] + 1e-6)


def temporal(out, t_rgb, dt, mm=None):
  """criterion.compute_temporal_rgb_loss (criterion.py:43-56)"""
  del dt
  pm = out['mask'].float() * (mm if mm is not None else 1.0)
  fw = (pm * out['occ_weight_map']).unsqueeze(-1).repeat(1, 3)
  return torch.sum(fw * torch.sqrt((out['rgb'] - t_rgb) ** 2 + 0.001 ** 2)) / (torch.sum(fw) + 1e-8)


def mono_objective_loss(ret, t, args, epoch, terms=ALL):
  """train.py:300-456 in plain torch, in the dtype of `ret` -> (loss, {name: value} in LOGGED's names).  Line numbers are train.py's."""
  ref, anc = ret['outputs_coarse_ref'], ret['outputs_coarse_anchor']
  ref_dy, anc_dy = ret['outputs_coarse_ref_dy'], ret['outputs_coarse_anchor_dy']
  dt = ref['rgb'].dtype
  zero = torch.zeros((), dtype=dt, device=ref['rgb'].device)
  divisor = epoch // args.init_decay_epoch                                                            # :302
  mm = t['motion_mask']
  log = {k: zero for k in LOGGED}
  if 'rgb' in terms:
    l = charb(ref['rgb'], t['rgb'], ref['mask'].float()) + temporal(anc, t['rgb'], dt)                # :304-307
    if epoch < args.init_decay_epoch:                                                                 # :309-316
      l = l + charb(ref['rgb_dy'], t['rgb'], ref['mask'].float() * mm)
    l = l + charb(ref_dy['rgb'], t['rgb'], ref_dy['mask'].float() * mm) / (10.0 ** divisor)            # :318-323
    l = l + temporal(anc_dy, t['rgb'], dt, mm) / (10.0 ** divisor)                                    # :324-328
    log['rgb'] = l
  pred_mask = ref['mask'].float()  # (.float() as train.py has it: in a float64 run the mask sums and their epsilons stay fp32, as in cases.mono_train_loss)
  if 'disp' in terms:                                                                                 # :331-342
    pred_disp = 1.0 / torch.clamp(ref['depth'], min=1e-2)
    log['disp'] = args.w_disp / (args.decay_rate ** divisor) * torch.sum(torch.abs(pred_disp - t['disp']) * pred_mask) / (torch.sum(pred_mask) + 1e-8)
  if 'flow' in terms:                                                                                 # :345-351, criterion.py:83-85
    nv = ref['render_flows'].shape[0]
    fm = (pred_mask[None, :, None] * t['masks'][:nv]).repeat(1, 1, 2)
    log['flow'] = args.w_flow / (args.decay_rate ** divisor) * torch.sum(torch.abs(ref['render_flows'] - t['flows'][:nv]) * fm) / (torch.sum(fm) + 1e-8)
  if 'cycle' in terms:                                                                                # :354-372
    w_cycle = min(0.5, args.w_cycle + divisor * args.cycle_factor) if args.anneal_cycle else args.w_cycle
    pa, pr = anc['pts_traj_anchor'], anc['pts_traj_ref']
    ow = anc['occ_weights'][None, ..., None].repeat(pa.shape[0], 1, 1, pa.shape[-1])
    log['cycle'] = w_cycle * torch.sum(torch.abs(pr - pa) * ow) / (torch.sum(ow) + 1e-8)
  if 'reg' in terms:                                                                                  # :375-398
    sf = anc['sf_seq']
    log['reg'] = args.w_reg * torch.mean(torch.abs(sf)) + args.w_reg * 0.5 * torch.mean(torch.pow(sf[:-1] - sf[1:], 2)) + \
        args.w_reg * torch.mean(torch.abs(sf[:, :, 1:, :] - sf[:, :, :-1, :]))
  wdy, wst = torch.sum(ref['weights_dy'], dim=-1), torch.sum(ref['weights_st'], dim=-1)               # :401-409
  ratio = wdy / torch.clamp(wdy + wst, min=1e-9)
  if 'entropy' in terms:                                                                              # :410-413
    log['entropy'] = args.w_skew_entropy * torch.mean(-(ratio * torch.log(ratio + 1e-9) + (1.0 - ratio) * torch.log(1.0 - ratio + 1e-9)))
  if 'distortion' in terms:                                                                           # :416-423
    sv = ref['s_vals']
    log['distortion'] = args.w_distortion * cases._distloss(ref['weights'][:, :-1], (sv[:, 1:] + sv[:, :-1]) * 0.5, sv[:, 1:] - sv[:, :-1])
  if 'static' in terms:                                                                               # :426-441
    ssm = (1.0 - t['static_mask']) * pred_mask * (1.0 - ratio).float().detach()
    l = charb(ref['rgb_static'], t['rgb'], ssm)
    if divisor > 4:
      sm2 = ssm * (ratio < 0.1).float()
      l = l + 0.1 * torch.sum(torch.abs(wdy * sm2.detach())) / torch.sum(sm2 + 1e-8)
    log['static'] = l
  loss = log['rgb'] + log['cycle'] + log['flow'] + log['disp'] + log['reg'] + log['entropy'] + log['distortion'] + log['static']  # :443-452
  log['loss'] = loss
  return loss, log


def reference_run(ret, tgt, args, epoch, terms, dtype, trainable=None):
  """the restatement and its autograd gradients on the CPU in `dtype` -> ({name: python float}, {leaf: grad or None})"""
  r, t, leaves = instantiate(ret, tgt, dtype, 'cpu', trainable)
  loss, log = mono_objective_loss(r, t, args, epoch, terms)
  if loss.requires_grad:
    loss.backward()
  return {k: float(v) for k, v in log.items()}, {k: v.grad for k, v in leaves.items()}


def kernel_run(device, ret, tgt, args, epoch, terms, trainable=None):
  from dynibar_amd import objective
  r, t, leaves = instantiate(ret, tgt, torch.float32, device, trainable)
  loss, logged = objective.MonoObjective(args)(r, t, epoch, terms)
  assert loss.dim() == 0 and logged.shape == (len(LOGGED),) and not logged.requires_grad
  if loss.requires_grad:
    loss.backward()
  return loss.detach().cpu(), logged.cpu(), {k: (None if v.grad is None else v.grad.cpu()) for k, v in leaves.items()}, r


def _limit(v32, v64):
  """twice the fp32 torch restatement's own largest deviation from float64 + 2e-6 of the largest magnitude (parity._accuracy_table's rule)"""
  return 2.0 * float((v32.double() - v64).abs().max()) + 2e-6 * float(v64.abs().max())


def check_objective(device, R, S, nv=6, T=4, epoch=0, terms=ALL, seed=7, args=None):
  """MonoObjective on `device` against the float64 restatement: each of the nine logged scalars and EVERY cotangent tensor, no element left
  out; the limit per tensor comes from the fp32 restatement's own error (_limit).  Also: exact zeros where torch has them on the zeroed tail
  samples and on masked rays, a second call bitwise equal, nothing NaN.  Returns the worst fraction of a limit used."""
  args = args or args_of()
  tag = f'objective R={R} S={S} nv={nv} epoch={epoch} terms={"full" if tuple(terms) == ALL else ",".join(terms)}'
  ret, tgt = make_case(R, S, nv, T, seed)
  assert_no_ties(ret)
  log64, g64 = reference_run(ret, tgt, args, epoch, terms, torch.float64)
  log32, g32 = reference_run(ret, tgt, args, epoch, terms, torch.float32)
  loss, logged, got, _ = kernel_run(device, ret, tgt, args, epoch, terms)
  loss2, logged2, got2, _ = kernel_run(device, ret, tgt, args, epoch, terms)
  assert torch.equal(loss, logged[0]), f'{tag}: loss and logged[0] differ'
  assert torch.equal(loss, loss2) and torch.equal(logged, logged2), f'{tag}: two calls differ in the loss / logged scalars'
  assert bool(torch.isfinite(logged).all()), f'{tag}: logged {logged.tolist()}'
  worst = 0.0
  for i, name in enumerate(LOGGED):
    v64, v32 = torch.tensor([log64[name]], dtype=torch.float64), torch.tensor([log32[name]], dtype=torch.float64)
    err, lim = float((logged[i].double() - v64).abs()), _limit(v32, v64)
    print(f'  {tag} logged[{name}] = {float(logged[i]):.9g} (float64 {log64[name]:.12g}, fp32 torch {log32[name]:.9g}) err {err:.2e} limit {lim:.2e}')
    if log64[name] == 0.0:
      assert float(logged[i]) == 0.0, f'{tag}: {name} must be exactly 0, got {float(logged[i])}'
      continue
    parity.record_margin(f'{tag} logged {name}', torch.tensor([err]), torch.tensor([lim]))
    worst = max(worst, err / lim)
    assert err <= lim, f'{tag}: logged {name} {float(logged[i])!r} vs float64 {log64[name]!r}: err {err:.3e} > limit {lim:.3e}'
  n_checked = 0
  for leaf in LEAVES:
    ref64, ref32, g, g2 = g64[leaf], g32[leaf], got[leaf], got2[leaf]
    if ref64 is None:
      assert g is None, f'{tag}: a gradient for {leaf} that the terms do not reach'
      continue
    assert g is not None, f'{tag}: no gradient for {leaf}'
    assert torch.equal(g, g2), f'{tag}: two calls differ in the cotangent of {leaf}'
    assert bool(torch.isfinite(g).all()), f'{tag}: non-finite cotangent of {leaf}'
    err, lim = float((g.double() - ref64).abs().max()), _limit(ref32, ref64)
    print(f'  {tag} d{leaf[0][15:]}.{leaf[1]}: err {err:.2e} limit {lim:.2e} (fp32 torch {float((ref32.double() - ref64).abs().max()):.2e}, max |g| {float(ref64.abs().max()):.2e})')
    parity.record_margin(f'{tag} cotangent {leaf[0]}.{leaf[1]}', torch.tensor([err]), torch.tensor([lim]))
    worst = max(worst, err / max(lim, 1e-300))
    assert err <= lim, f'{tag}: cotangent of {leaf}: max err {err:.3e} > limit {lim:.3e}'
    zeros = ref64 == 0
    assert bool((g[zeros] == 0).all()), f'{tag}: cotangent of {leaf} is non-zero at {int((g[zeros] != 0).sum())} elements where torch has exact zeros'
    n_checked += 1
  assert n_checked > 0, f'{tag}: no cotangent was checked'
  return worst


def check_exact_zeros(device, R=37, S=20, seed=8):
  """sign(0) = 0: with the magnitude term of sf_seq and the consistency term alone, the cotangents on the zeroed tail samples are exactly 0
  (torch.abs's gradient at 0); on rays whose mask is 0 the colour cotangents are exactly 0; inputs without requires_grad get no gradient."""
  args = args_of()
  ret, tgt = make_case(R, S, 6, 4, seed)
  nt = n_tail(S)
  assert nt > 0
  for terms, names in ((('reg',), ('sf_seq',)), (('cycle',), ('pts_traj_ref', 'pts_traj_anchor'))):
    _, g64 = reference_run(ret, tgt, args, 0, terms, torch.float64)
    _, _, got, _ = kernel_run(device, ret, tgt, args, 0, terms)
    for k in names:
      g, ref = got[('outputs_coarse_anchor', k)], g64[('outputs_coarse_anchor', k)]
      tail_ref = ref[:, :, S - nt + 1:] if k == 'sf_seq' else ref[:, :, S - nt:]  # (the first tail sample of sf_seq has a non-zero spatial neighbour)
      tail = g[:, :, S - nt + 1:] if k == 'sf_seq' else g[:, :, S - nt:]
      assert bool((tail_ref == 0).all()), 'the yardstick itself is not zero on the tail'
      assert bool((tail == 0).all()), f'{k}: {int((tail != 0).sum())} non-zero cotangents on the zeroed tail samples (sign(0) must be 0)'
      assert bool((g[ref == 0] == 0).all()) and bool((g[ref != 0] != 0).all()), f'{k}: zero pattern differs from torch'
  _, _, got, r = kernel_run(device, ret, tgt, args, 0, ALL)
  dead = ~r['outputs_coarse_ref']['mask'].cpu()
  assert int(dead.sum()) > 0
  for k in ('rgb', 'rgb_dy', 'rgb_static', 'depth'):
    assert bool((got[('outputs_coarse_ref', k)][dead] == 0).all()), f'{k}: non-zero cotangent on a ray with mask 0'
  assert bool((got[('outputs_coarse_ref', 'render_flows')][:, dead] == 0).all())
  some = (('outputs_coarse_ref', 'rgb'), ('outputs_coarse_anchor', 'sf_seq'))
  _, _, got, _ = kernel_run(device, ret, tgt, args, 0, ALL, trainable=some)
  assert set(got) == set(some) and all(v is not None for v in got.values())
  _, g64 = reference_run(ret, tgt, args, 0, ALL, torch.float64, trainable=some)
  for k in some:
    assert float((got[k].double() - g64[k]).abs().max()) <= 2e-6 * float(g64[k].abs().max())


def distloss_quadratic(w, m, interval):
  """the definition: sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 interval_i, mean over the rays"""
  return ((w[..., :, None] * w[..., None, :] * (m[..., :, None] - m[..., None, :]).abs()).sum((-1, -2)) + (w ** 2 * interval).sum(-1) / 3.0).mean()


def check_distloss(device, S, R=5, seed=3):
  """eff_distloss_native alone: value and the gradients to w, m and interval against cases._distloss in float64; the limit as in _limit"""
  from dynibar_amd import objective
  g = torch.Generator().manual_seed(seed + S)
  w = torch.rand(R, S + 1, generator=g) ** 2
  edges = torch.sort(torch.rand(R, S + 1, generator=g), dim=-1).values
  m, d = (edges[:, 1:] + edges[:, :-1]) * 0.5, edges[:, 1:] - edges[:, :-1]

  def run(fn, dtype, dev):
    ws, ms, ds = (x.to(dtype).to(dev).clone().requires_grad_(True) for x in (w, m, d))
    loss = fn(ws[:, :-1], ms, ds)  # (w is a slice, as train.py passes it)
    loss.backward()
    return loss.detach().cpu(), [x.grad.cpu() for x in (ws, ms, ds)]

  l64, g64 = run(cases._distloss, torch.float64, 'cpu')
  l32, g32 = run(cases._distloss, torch.float32, 'cpu')
  l, got = run(objective.eff_distloss_native, torch.float32, device)
  l2, got2 = run(objective.eff_distloss_native, torch.float32, device)
  assert torch.equal(l, l2) and all(torch.equal(a, b) for a, b in zip(got, got2)), f'distloss S={S}: two calls differ'
  for what, a, b32, b64 in [('value', l, l32, l64)] + [(f'd{n}', a, b, c) for n, a, b, c in zip(('w', 'm', 'interval'), got, g32, g64)]:
    err, lim = float((a.double() - b64).abs().max()), _limit(b32, b64)
    parity.record_margin(f'eff_distloss_native S={S} {what}', torch.tensor([err]), torch.tensor([lim]))
    assert err <= lim, f'eff_distloss_native S={S} {what}: err {err:.3e} > limit {lim:.3e}'
