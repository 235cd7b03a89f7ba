"""Seeded test cases shared by the golden generator, the oracle tests and the GPU parity tests."""
import numpy as np
import torch

from dynibar_amd import synthetic as syn

NUM_FRAMES = 24
REF_FRAME = 11
NUM_BASIS = 6


def t(x):
  return torch.from_numpy(np.ascontiguousarray(x))


def scene_case(name):
  """name -> (scene dict of torch tensors, ray_o, ray_d, uv, pixel ids).  'edge_<V>_<n_static>_<R>': an extreme shape (1-2 views, a single ray)."""
  if name.startswith('edge_'):
    v, ns, r = (int(x) for x in name.split('_')[1:])
    return _scene_of(dict(seed=61, H=32, W=48, V=v, n_static=ns, smooth=True), r)
  cfg = {
      # small, smooth maps: well-conditioned parity
      'small': dict(seed=1, H=48, W=64, V=7, n_static=8, smooth=True, R=6),
      # wide baselines / rotations: many out-of-bounds and behind-camera samples
      'harsh': dict(seed=2, H=40, W=56, V=5, n_static=11, smooth=True, R=5, t_scale=3.0, r_scale=1.2, near=0.3, far=6.0),
      # the same scene with enough rays for several workgroups and several planning segments of the ragged dense-rows flavour (48 x 64 = 3072 points x 11 static views)
      'harsh_many': dict(seed=2, H=40, W=56, V=5, n_static=11, smooth=True, R=48, t_scale=3.0, r_scale=1.2, near=0.3, far=6.0),
      # white-noise maps (the bench's data distribution): ill-conditioned bilinear taps, looser tolerance
      'noise': dict(seed=3, H=32, W=48, V=7, n_static=8, smooth=False, R=4),
      # view counts that exercise the other lane-segment widths of the network kernels (4 and 32 lanes per point)
      'few': dict(seed=5, H=32, W=48, V=3, n_static=4, smooth=True, R=5),
      'many': dict(seed=6, H=32, W=48, V=13, n_static=20, smooth=True, R=3),
      # BASELINE configs[4] (stress): 16 views in both branches, rendered with 128 + 128 samples
      # configs/train_kid-running.txt shape: 7 time-offset + num_vv = 3 virtual dynamic views, 15 static views (render_monocular_bt.py:113-201)
      'kid': dict(seed=8, H=32, W=48, V=10, n_static=15, smooth=True, R=5),
      'stress': dict(seed=7, H=32, W=48, V=16, n_static=16, smooth=True, R=4),
      # the training shape of configs/train_kid-running.txt at a size the oracle's autograd runs on the device in seconds: 64 samples,
      # 7 + 3 dynamic views at the reference and at the anchor frame, 15 static views, hundreds of rays (tests/parity.check_train_mono_large)
      'train_large': dict(seed=31, H=144, W=256, V=10, n_static=15, smooth=True, R=256),
      # BASELINE configs[0] at its stated size: 288 x 512 images, 72 x 128 x 32 white-noise feature maps, 8 static source
      # views, 512 rays x 64 samples -- the one named configuration whose size an oracle run affords in full (seconds)
      'config0': dict(seed=40, H=288, W=512, V=7, n_static=8, smooth=False, R=512),
      # shapes on which the reference's torch.cross WITHOUT dim (render_ray.py:375, :392) does not cross over xyz: exactly 3 static source views, a chunk
      # of exactly 3 rays, (with CROSS_AXIS_SAMPLES) 3 samples per ray, and the two combinations that decide the precedence (tests/golden/cross_axis.npz)
      'cross_views': dict(seed=51, H=32, W=48, V=5, n_static=3, smooth=True, R=5),
      'cross_rays': dict(seed=52, H=32, W=48, V=5, n_static=8, smooth=True, R=3),
      'cross_samples': dict(seed=53, H=32, W=48, V=5, n_static=8, smooth=True, R=4),
      'cross_rays_views': dict(seed=54, H=32, W=48, V=5, n_static=3, smooth=True, R=3),
      'cross_rays_samples': dict(seed=55, H=32, W=48, V=5, n_static=8, smooth=True, R=3),
      # 24 feature maps: 64 % (F / 4) != 0, the width at which dyn_project_gather falls back to its row-order kernel
      'wide24': dict(seed=9, H=32, W=48, V=5, n_static=6, smooth=True, R=5, F=24),
  }[name]
  return _scene_of(cfg, cfg.pop('R'))


def _scene_of(cfg, R):
  seed = cfg['seed']
  sc = syn.make_scene(**cfg)
  fine = syn.make_scene(**dict(cfg, tag=1))  # fine-stage feature maps come from a second encoder
  pix = syn.sample_pixels(seed, cfg['H'], cfg['W'], R)
  o, d, uv = syn.pixel_rays(sc['camera'], pix)
  scene = {k: t(v) for k, v in sc.items()}
  scene['featmaps_fine'] = t(fine['featmaps'])
  scene['static_featmaps_fine'] = t(fine['static_featmaps'])
  return scene, t(o), t(d), t(uv), pix


# samples per ray of the cross-axis cases
CROSS_AXIS_SAMPLES = {'cross_views': 8, 'cross_rays': 8, 'cross_samples': 3, 'cross_rays_views': 8, 'cross_rays_samples': 3}


def model_weights(seed=0):
  """numpy state dicts for the six DynibarFF nets + DCT bases (model.py:33-101)."""
  m = {
      'net_coarse_st': syn.make_weights('static', seed),
      'net_coarse_dy': syn.make_weights('dynamic', seed),
      'net_fine_st': syn.make_weights('static', seed + 100),
      'net_fine_dy': syn.make_weights('dynamic', seed + 100),
      'motion_mlp': syn.make_weights('motion', seed, num_basis=NUM_BASIS),
      'motion_mlp_fine': syn.make_weights('motion', seed + 100, num_basis=NUM_BASIS),
  }
  return m


def model_weights_trained(seed=3):
  """Weights at the scale of a trained model rather than of an initialisation: every matrix 1.4x Kaiming, biases up to +-1, LayerNorm
  gains around 3, density heads 5x: density logits spanning -40..+25 on the test scenes (what the split-product engine must hold
  1e-4 (+1e-4 relative) on)."""
  kw = dict(gain=1.4, bias=1.0, head_gain=5.0, ln_gain=3.0)
  m = {
      'net_coarse_st': syn.make_weights('static', seed, **kw),
      'net_coarse_dy': syn.make_weights('dynamic', seed, **kw),
      'net_fine_st': syn.make_weights('static', seed + 100, **kw),
      'net_fine_dy': syn.make_weights('dynamic', seed + 100, **kw),
      'motion_mlp': syn.make_weights('motion', seed, num_basis=NUM_BASIS, gain=1.3, bias=0.5),
      'motion_mlp_fine': syn.make_weights('motion', seed + 100, num_basis=NUM_BASIS, gain=1.3, bias=0.5),
  }
  return m


def anchor_case(scene, num_vv=2, anchor_shift=1):
  """Anchor-time inputs of the monocular training path for a scene_case scene: the anchor frame's source set is the scene's own
  source set rolled by two views (different images / cameras / feature maps per slot), its time offsets are a different list.
  Returns (scene with anchor_* entries, (ref, anchor) frame indices, time embeddings, time offsets)."""
  V = scene['src_rgbs'].shape[1]
  fidx, temb, toff = time_args(V)
  toff = toff[:V - num_vv]
  aidx = fidx + anchor_shift
  aoff = ([-2, -1, 1, 2, 3, -3, 0] * 3)[:V - num_vv]
  sc = dict(scene)
  sc['anchor_src_rgbs'] = torch.roll(scene['src_rgbs'], 2, dims=1).contiguous()
  sc['anchor_src_cameras'] = torch.roll(scene['src_cameras'], 2, dims=1).contiguous()
  sc['featmaps_anchor'] = torch.roll(scene['featmaps'], 2, dims=0).contiguous()
  temb_a = torch.tensor([aidx / float(NUM_FRAMES)], dtype=torch.float32)
  return sc, (fidx, aidx), (temb, temb_a), (toff, aoff)


ENCODER_CASES = {
    'small': dict(seed=11, N=2, H=40, W=56), 'odd': dict(seed=12, N=3, H=37, W=50), 'wide': dict(seed=13, N=1, H=64, W=160),
    'tiny': dict(seed=14, N=2, H=21, W=30),  # tiny: the emulator's training-form case (no golden)
    # the shapes the encoder runs in production (eval_nvidia.py: 18 source views; train.py: 10) and shapes chosen for how k_enc_conv splits the
    # N * Hout output rows over the workgroups (tests/encoder_checks.py:conv_split states what each reaches)
    'eval': dict(seed=15, N=18, H=288, W=512), 'train': dict(seed=16, N=10, H=288, W=512),
    'ragged': dict(seed=17, N=7, H=147, W=97), 'just_over': dict(seed=18, N=3, H=201, W=131),
    'many': dict(seed=19, N=300, H=16, W=16), 'min': dict(seed=20, N=1, H=16, W=16), 'nine': dict(seed=22, N=9, H=16, W=16),
    'tall': dict(seed=26, N=2, H=64, W=16),
    'odd_w': dict(seed=21, N=1, H=33, W=45),  # odd width, pinned to the real reference by tests/golden/encoder_odd_w.npz
    # low-contrast frames (tests/encoder_checks.py:check_encoder_conditioning): |mean| / std of a conv1 channel in the hundreds, or no variance at all
    'dim': dict(seed=23, N=2, H=288, W=512, contrast=0.05), 'flat': dict(seed=24, N=2, H=288, W=512, noise=0.01),
    'const': dict(seed=25, N=2, H=288, W=512, noise=0.0),
}


def encoder_case(name='small', shape=None):
  """Seeded image batch [N,H,W,3] in [0,1] for the feature encoder (the data loaders' source images) and the encoder weights.
  shape = (N, H, W) overrides the case's size (the emulator runs the low-contrast cases on thumbnails)."""
  cfg = dict(ENCODER_CASES[name])
  if shape is not None:
    cfg['N'], cfg['H'], cfg['W'] = shape
  rng = np.random.default_rng([cfg['seed'], 5])
  if 'noise' in cfg:  # uniform noise of the given contrast about mid-grey (0: a constant image)
    img = 0.5 + cfg['noise'] * (rng.uniform(0.0, 1.0, (cfg['N'], cfg['H'], cfg['W'], 3)) - 0.5)
    return t(img.astype(np.float32)), syn.make_encoder_weights(cfg['seed'])
  yy, xx = np.meshgrid(np.linspace(0, 1, cfg['H']), np.linspace(0, 1, cfg['W']), indexing='ij')
  imgs = []
  for n in range(cfg['N']):
    ph = rng.uniform(0, 6.28, (3, 4))
    fr = rng.uniform(2, 9, (3, 4))
    img = np.stack([0.5 + 0.25 * np.sin(fr[c, 0] * xx + ph[c, 0]) * np.cos(fr[c, 1] * yy + ph[c, 1]) + 0.2 * np.sin(fr[c, 2] * (xx + yy) + ph[c, 2])
                    for c in range(3)], -1) + 0.05 * rng.standard_normal((cfg['H'], cfg['W'], 3))
    imgs.append(np.clip(img, 0.0, 1.0))
  imgs = np.stack(imgs, 0)
  if 'contrast' in cfg:  # the same frame, dim: its contrast about mid-grey reduced
    imgs = 0.5 + cfg['contrast'] * (imgs - 0.5)
  return t(imgs.astype(np.float32)), syn.make_encoder_weights(cfg['seed'])


def time_args(n_views):
  """(frame_idx, time_embedding[1], time_offset list) like eval_nvidia.py:323-329."""
  offs = [-3, -2, -1, 0, 1, 2, 3][:n_views] if n_views <= 7 else [((i * 5) % 7) - 3 for i in range(n_views)]
  return REF_FRAME, torch.tensor([REF_FRAME / float(NUM_FRAMES)], dtype=torch.float32), offs


def bootstrap_case(kid):
  """The static bootstrap iteration of tests/parity.check_static_bootstrap_step and its golden (tests/golden/train_static.npz):
  scene name, samples, num_vv, (anti_alias_pooling, mask_rgb), seeded ground-truth colours [R,3] and static-region mask [R] (ray_batch['rgb'],
  ray_batch['static_mask'] of train.py:180-186)."""
  name = 'kid' if kid else 'small'
  scene, o, d, uv, _ = scene_case(name)
  g = torch.Generator().manual_seed(77)
  n = o.shape[0]
  gt = torch.rand(n, 3, generator=g)
  static_mask = (torch.rand(n, generator=g) < 0.3).float()
  return dict(name=name, S=32, num_vv=3 if kid else 0, aa=0 if kid else 1, mask_rgb=1 if kid else 0, gt=gt, static_mask=static_mask)


def charbonnier(x, y, mask, eps=0.001):
  """utils.img2charbonier (utils.py:32-39) with TINY_NUMBER = 1e-6"""
  return torch.sum(torch.sqrt((x - y) ** 2 + eps ** 2) * mask.unsqueeze(-1)) / (torch.sum(mask) * x.shape[-1] + 1e-6)


# ---- the reference's main-loop loss (train.py:302-446) restated for the gradient goldens / tests (test infrastructure) ------------------
def train_batch_targets(n_rays, n_flow_views=6, seed=91):
  """Seeded stand-ins for the data loader's supervision in ray_batch (train.py:302-446): rgb, disp, flows, masks, motion_mask, static_mask."""
  g = torch.Generator().manual_seed(seed)
  return dict(rgb=torch.rand(n_rays, 3, generator=g), disp=0.05 + 0.5 * torch.rand(n_rays, generator=g),
              flows=4.0 * torch.randn(n_flow_views, n_rays, 2, generator=g), masks=(torch.rand(n_flow_views, n_rays, 1, generator=g) < 0.8).float(),
              motion_mask=(torch.rand(n_rays, generator=g) < 0.5).float(), static_mask=(torch.rand(n_rays, generator=g) < 0.3).float())


def _distloss(w, m, interval):
  """eff_distloss_native of the third-party package torch_efficient_distloss (environment_dynibar.yml:17, un-pinned; absent here):
  its published O(N) form of the mip-NeRF-360 distortion loss."""
  loss_uni = (1.0 / 3.0) * (interval * w.pow(2)).sum(dim=-1).mean()
  wm = w * m
  w_cs, wm_cs = w.cumsum(dim=-1), wm.cumsum(dim=-1)
  loss_bi = 2.0 * (wm[..., 1:] * w_cs[..., :-1] - w[..., 1:] * wm_cs[..., :-1]).sum(dim=-1).mean()
  return loss_bi + loss_uni


def mono_train_loss(ret, tgt, terms=('rgb', 'disp', 'flow', 'cycle', 'reg', 'entropy', 'distortion', 'static'), epoch=0):
  """train.py:302-446 with configs/train_kid-running.txt's weights (w_disp 0.1, w_flow 0.01, w_cycle 0.1, w_reg 0.05, w_skew_entropy 5e-4,
  w_distortion 1e-3, decay_rate 10, init_decay_epoch 400).  `terms` selects a subset (each with its train.py weight)."""
  ref, anc = ret['outputs_coarse_ref'], ret['outputs_coarse_anchor']
  ref_dy, anc_dy = ret['outputs_coarse_ref_dy'], ret['outputs_coarse_anchor_dy']
  divisor = epoch // 400
  dev = ref['rgb'].device
  t = {k: v.to(dev) for k, v in tgt.items()}
  crit = lambda out, mm=None: charbonnier(out['rgb'], t['rgb'], out['mask'].float() * (mm if mm is not None else 1.0))

  def temporal(out, mm=None):
    pm = out['mask'].float() * (mm if mm is not None else 1.0)
    fw = (pm * out['occ_weight_map']).unsqueeze(-1).repeat(1, 3)
    return torch.sum(fw * torch.sqrt((out['rgb'] - t['rgb']) ** 2 + 0.001 ** 2)) / (torch.sum(fw) + 1e-8)

  loss = 0.0
  if 'rgb' in terms:
    l = crit(ref) + temporal(anc)
    if epoch < 400:
      l = l + charbonnier(ref['rgb_dy'], t['rgb'], ref['mask'].float() * t['motion_mask'])
    l = l + crit(ref_dy, t['motion_mask']) / (10.0 ** divisor) + temporal(anc_dy, t['motion_mask']) / (10.0 ** divisor)
    loss = loss + l
  pred_mask = ref['mask'].float()
  if 'disp' in terms:
    pred_disp = 1.0 / torch.clamp(ref['depth'], min=1e-2)
    loss = loss + 0.1 / (10.0 ** divisor) * torch.sum(torch.abs(pred_disp - t['disp']) * pred_mask) / (torch.sum(pred_mask) + 1e-8)
  if 'flow' in terms:
    nv = ref['render_flows'].shape[0]  # min(6, dynamic views) (render_ray.py:1077-1082)
    fm = (pred_mask[None, :, None] * t['masks'][:nv]).repeat(1, 1, 2)
    loss = loss + 0.01 / (10.0 ** divisor) * torch.sum(torch.abs(ref['render_flows'] - t['flows'][:nv]) * fm) / (torch.sum(fm) + 1e-8)
  if 'cycle' in terms:
    pa, pr = anc['pts_traj_anchor'], anc['pts_traj_ref']
    ow = anc['occ_weights'][None, ..., None].repeat(pa.shape[0], 1, 1, pa.shape[-1])
    loss = loss + 0.1 * torch.sum(torch.abs(pr - pa) * ow) / (torch.sum(ow) + 1e-8)
  if 'reg' in terms:
    sf = anc['sf_seq']
    loss = loss + 0.05 * torch.mean(torch.abs(sf)) + 0.05 * 0.5 * torch.mean(torch.pow(sf[:-1] - sf[1:], 2)) + \
        0.05 * torch.mean(torch.abs(sf[:, :, 1:, :] - sf[:, :, :-1, :]))
  wdy, wst = torch.sum(ref['weights_dy'], dim=-1), torch.sum(ref['weights_st'], dim=-1)
  ratio = wdy / torch.clamp(wdy + wst, min=1e-9)
  if 'entropy' in terms:
    loss = loss + 5e-4 * torch.mean(-(ratio * torch.log(ratio + 1e-9) + (1.0 - ratio) * torch.log(1.0 - ratio + 1e-9)))
  if 'distortion' in terms:
    sv = ref['s_vals']
    loss = loss + 1e-3 * _distloss(ref['weights'][:, :-1], (sv[:, 1:] + sv[:, :-1]) * 0.5, sv[:, 1:] - sv[:, :-1])
  if 'static' in terms:
    ssm = (1.0 - t['static_mask']) * pred_mask * (1.0 - ratio).float().detach()
    loss = loss + charbonnier(ref['rgb_static'], t['rgb'], ssm)
  return loss


def grad_digest(g, seed=5):
  """A gradient tensor -> small fingerprint: four seeded random projections, the largest magnitude and the first 32 values (keeps the
  golden file small while any wrong element moves a projection)."""
  g = g.detach().double().reshape(-1).cpu()
  gen = torch.Generator().manual_seed(seed)
  pr = torch.stack([(g * torch.randn(g.numel(), generator=gen, dtype=torch.float64)).sum() for _ in range(4)])
  return dict(proj=pr, absmax=g.abs().max().reshape(1), head=g[:32].clone(), l1=g.abs().sum().reshape(1))


MONO_TRAIN_LOSSES = {'full': ('rgb', 'disp', 'flow', 'cycle', 'reg', 'entropy', 'distortion', 'static'), 'flow': ('flow',), 'cycle': ('cycle',),
                     'reg': ('reg',), 'rgb': ('rgb',)}


CRITERION_SEEDS = (0, 1)


def criterion_cases(m, seed, R=37, V=3):
  """The loss helpers train.py imports, on seeded inputs: [(name, loss of module m, leaves)] (tests/test_criterion.py and its golden,
  tests/golden/criterion.npz).  m: dynibar_amd.criterion or the reference's ibrnet/criterion.py."""
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32)
  outputs = dict(rgb=r(R, 3).requires_grad_(), mask=(r(R) > 0.2), occ_weight_map=r(R).requires_grad_())
  batch = dict(rgb=r(R, 3))
  mm, flow, gt_flow, gt_mask = (r(R) > 0.3).float(), r(V, R, 2).requires_grad_(), r(V, R, 2), (r(V, R, 1) > 0.4).float()
  return [
      ('Criterion', lambda: m.Criterion()(outputs, batch), [outputs['rgb']]),
      ('Criterion+motion_mask', lambda: m.Criterion()(outputs, batch, mm), [outputs['rgb']]),
      ('temporal_rgb', lambda: m.compute_temporal_rgb_loss(outputs, batch, mm), [outputs['rgb'], outputs['occ_weight_map']]),
      ('temporal_rgb no mask', lambda: m.compute_temporal_rgb_loss(outputs, batch), [outputs['rgb'], outputs['occ_weight_map']]),
      ('rgb', lambda: m.compute_rgb_loss(outputs['rgb'], batch, outputs['mask'].float()), [outputs['rgb']]),
      ('entropy', lambda: m.compute_entropy(outputs['occ_weight_map']), [outputs['occ_weight_map']]),
      ('flow', lambda: m.compute_flow_loss(flow, gt_flow, gt_mask), [flow]),
  ]


# the reference's argument sets (tests/test_model_adapter.py) and the module constructions whose structure tests/golden/reference_modules.json records
MODULE_ARG_SETS = {'nvidia_eval': dict(anti_alias_pooling=1, mask_rgb=0), 'kid_running': dict(anti_alias_pooling=0, mask_rgb=1)}
MODULE_ATTRS = ('anti_alias_pooling', 'mask_rgb', 'shift', 'sf_mag_div', 'num_basis')


def load_golden(golden_dir, name):
  """tests/golden/<name> as a dict of arrays; a golden stored in parts (<stem>.part<i>.npz, tests/golden/make_golden.py:save_parts) is merged."""
  import glob
  import os
  path = os.path.join(golden_dir, name)
  if os.path.exists(path):
    return dict(np.load(path))
  stem = path[:-len('.npz')] if path.endswith('.npz') else path
  parts = sorted(glob.glob(stem + '.part*.npz'), key=lambda p: int(p[len(stem) + len('.part'):-len('.npz')]))
  assert parts, f'no golden {name} in {golden_dir}'
  out = {}
  for p in parts:
    out.update(np.load(p))
  return out


# ---- seeded inputs of the per-ray kernels' edge tests (tests/parity.py: check_fine_samples_case, check_composite_case, ...) -----------------
# (R, S, N) of k_fine_samples: the smallest legal problem, a second workgroup holding one ray, N != S, the largest problem of the 64-ray
# LDS split (S = 256, N = 64: 143.5 KiB), the 32-ray split (S = 256 with N = 128 / 255)
FINE_SAMPLE_SHAPES = [(1, 3, 2), (5, 4, 3), (65, 64, 17), (130, 64, 65), (70, 128, 128), (33, 256, 64), (33, 256, 128), (40, 256, 255)]
FINE_SAMPLE_SHAPE_LARGE = (4099, 64, 64)  # 65 workgroups, the last one holding three rays (device only)
FINE_SAMPLE_PDF_SHAPES = [(5, 4, 3), (130, 64, 65), (33, 256, 128)]  # the shapes the sample_pdf export is run on
FINE_WEIGHT_KINDS = ('composite', 'zero', 'onehot03', 'onehot1', 'ends', 'spike', 'dup_depth')
FINE_U_KINDS = ('u01', 'knots', 'knots_down')
RAMP_DETECTOR_SHAPES = [(128, 64), (256, 128), (64, 32)]  # (S, N) with S - 2 = 2 (N - 1): every second knot of a uniform cdf is a ramp value


def _gen(*key):
  return torch.Generator().manual_seed(int(np.random.SeedSequence(list(key)).generate_state(1)[0]))


def fine_sample_depths(R, S, inv_uniform, seed=0):
  """Strictly increasing coarse depths [R,S], uniform in disparity or in depth like sample_along_camera_ray's, near / far varying by ray."""
  g = _gen(seed, R, S, 1)
  near = 0.5 + 0.2 * torch.rand(R, 1, generator=g)
  far = 8.0 + 2.0 * torch.rand(R, 1, generator=g)
  t = torch.arange(S, dtype=torch.float32)[None] / float(S - 1)
  if inv_uniform:
    return 1.0 / (1.0 / near + t * (1.0 / far - 1.0 / near))
  return near + t * (far - near)


def fine_sample_weights(kind, R, S, seed=0):
  """Coarse weights [R,S] of one of FINE_WEIGHT_KINDS ('dup_depth' uses the composite-like weights; the depths carry its edge)."""
  g = _gen(seed, R, S, 2)
  w = torch.zeros(R, S)
  if kind in ('composite', 'dup_depth', 'u01', 'knots', 'knots_down'):  # softplus of 3 N(0,1) logits through the compositing formula
    a = 1.0 - torch.exp(-torch.nn.functional.softplus(3.0 * torch.randn(R, S, generator=g)))
    T = torch.cumprod(torch.cat([torch.ones(R, 1), 1.0 - a + 1e-10], dim=1), dim=1)[:, :-1]
    w = a * T
  elif kind in ('onehot03', 'onehot1'):  # all mass in one interior sample
    w[torch.arange(R), torch.randint(1, S - 1, (R,), generator=g)] = 0.3 if kind == 'onehot03' else 1.0
  elif kind == 'ends':  # mass only at the two samples sample_pdf excludes
    w[:, 0] = 0.5
    w[:, -1] = 0.5
  elif kind == 'spike':
    w = torch.full((R, S), 1e-12)
    w[:, S // 2 if S > 3 else 1] = 0.9
  else:
    assert kind == 'zero', kind
  return w.contiguous()


def fine_sample_u(kind, R, N, cdf=None, seed=0):
  """u [R,N] in [0, 1]: 'rand'; 'u01' (a column of 0 and a column of 1 - ulp); 'knots' (values of the given cdf [R,M+1] themselves);
  'knots_down' (the same values moved one ulp towards 0)."""
  g = _gen(seed, R, N, 3)
  u = torch.rand(R, N, generator=g)
  if kind == 'u01':
    u[:, 0] = 0.0
    u[:, -1] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
  elif kind in ('knots', 'knots_down'):
    idx = torch.randint(0, cdf.shape[1], (R, N), generator=g)
    u = torch.gather(cdf, 1, idx).clamp(max=1.0)
    if kind == 'knots_down':
      u = torch.nextafter(u, torch.zeros_like(u))
  else:
    assert kind == 'rand', kind
  return u.contiguous()


def linspace01_restated(N, fused=True):
  """csrc/dyn_geometry.hip:linspace01 restated in NumPy: n * step below N / 2, fma(-step, N - 1 - n, 1) from there on (the 24 x 10 bit
  product and its difference from 1 are exact in float64, so the one rounding to fp32 is the fused operation's).  fused=False: the
  product rounded to fp32 first -- the kernels' formula before the ramp was settled, and what a torch build without FMA kernels gives."""
  f = np.float32
  step = f(1.0) / f(N - 1)
  n = np.arange(N)
  lo = n.astype(f) * step
  k = (N - 1 - n)
  hi = (1.0 - np.float64(step) * k.astype(np.float64)).astype(f) if fused else f(1.0) - k.astype(f) * step
  return torch.from_numpy(np.where(n < N // 2, lo, hi).astype(f))


def kernel_cdf_restated(w):
  """k_fine_samples' cdf recipe restated in NumPy: interior weights [R,M] (in sample_pdf's order) -> cdf [R,M+1].  1e-5 added in fp32, the
  total summed sequentially in double and rounded once, every quotient rounded to fp32, a sequential double prefix sum rounded per knot."""
  wj = (w.float() + 1e-5).numpy()
  total = np.cumsum(wj.astype(np.float64), axis=1)[:, -1:].astype(np.float32)
  pdf = (wj / total).astype(np.float32)
  cdf = np.cumsum(pdf.astype(np.float64), axis=1).astype(np.float32)
  return torch.from_numpy(np.concatenate([np.zeros_like(cdf[:, :1]), cdf], axis=1))


COMPOSITE_SHAPES = [(1, 2), (3, 63), (4, 64), (5, 65), (9, 128), (6, 129), (5, 200), (3, 256), (1030, 64)]  # (R, S)
COMPOSITE_MODIFIERS = ('plain', 'opaque', 'masked', 'chunk_edge', 'count_head', 'count_tail')


def composite_case(R, S, seed=0, modifier='plain'):
  """raw_dy, raw_st [R,S,4], z [R,S] sorted, pm_dy, pm_st [R,S] bool for k_composite.  Modifiers: 'opaque' (every 7th dynamic logit 50, every 11th
  static logit 1e4), 'masked' (every logit -1e9), 'chunk_edge' (a logit of 40 at samples 63, 64, 127, 128 -- either side of the kernel's 64-sample
  chunks -- of every second ray), 'count_head' / 'count_tail' (exactly 7, 8 or 9 observed samples per ray and branch, every pair of counts
  within nine rays, at the start / at the end of the ray; the ray mask is `count > 8`)."""
  g = _gen(seed, R, S, 4)
  raw_dy = torch.randn(R, S, 4, generator=g) * torch.tensor([1, 1, 1, 3.0])
  raw_st = torch.randn(R, S, 4, generator=g) * torch.tensor([1, 1, 1, 3.0])
  z = torch.sort(torch.rand(R, S, generator=g) * 10 + 0.5, dim=1)[0]
  pm_dy = torch.rand(R, S, generator=g) > 0.7
  pm_st = torch.rand(R, S, generator=g) > 0.9
  if modifier == 'opaque':
    raw_dy[:, ::7, 3] = 50.0
    raw_st[:, 3::11, 3] = 1e4
  elif modifier == 'masked':
    raw_dy[..., 3] = -1e9
    raw_st[..., 3] = -1e9
  elif modifier == 'chunk_edge':
    for s in (63, 64, 127, 128):
      if s < S:
        raw_dy[0::2, s, 3] = 40.0
        raw_st[1::4, s, 3] = 40.0
  elif modifier in ('count_head', 'count_tail'):
    pm_dy[:] = False
    pm_st[:] = False
    for r in range(R):
      n, m = min(7 + (r + 1) % 3, S), min(7 + ((r + 1) // 3) % 3, S)  # ray 0: (8, 7), ray 1: (9, 7), ray 2: (7, 8), ray 3: (8, 8), ...
      if modifier == 'count_head':
        pm_dy[r, :n] = True
        pm_st[r, :m] = True
      else:
        pm_dy[r, S - n:] = True
        pm_st[r, S - m:] = True
  else:
    assert modifier == 'plain', modifier
  return raw_dy, raw_st, z, pm_dy, pm_st
