"""Shared by tests/emu/test_emu_points_two_wave.py and tests/test_gpu_points_two_wave.py: the same rays through the point networks in one call and
in two, so that they land in different waves and workgroups of the point kernel (8 row tiles per workgroup, tile = ray * tiles_per_ray + k)."""
import torch
import torch.nn.functional as F

import parity
from dynibar_amd import ops


def static_split_outputs(device, name='small', S=64, R=5, cut=2):
  """DynibarStatic on R rays at once, and on rays [0, cut) and [cut, R) in two calls -> (raw of the one call, raw of the two calls joined)."""
  scene, o, d, sd, _, st = parity.static_inputs(name, S, R)
  sdev = parity.to_dev(scene, device)
  views = ops.SourceViews(sdev['camera'], sdev['static_src_rgbs'], sdev['static_src_cameras'], sdev['static_featmaps'])
  net = ops.StaticNet(parity._weights('init')['net_coarse_st'], device, True, False)

  def run(a, b):
    dv = lambda x: x[a:b].contiguous().to(device)
    return parity.cpu(net(views, dv(o), dv(d), dv(st['pts']), dv(st['rgb_feat']), dv(st['ray_diff']), dv(st['mask']))).clone()

  return run(0, R), torch.cat([run(0, cut), run(cut, R)], 0)


def dynamic_split_outputs(device, name='small', S=64, R=5, cut=2, shift=5.0):
  di = parity.dynamic_inputs(name, S, R)
  net = ops.DynamicNet(parity._weights('init')['net_coarse_dy'], device, shift=shift)
  temb = di['temb'].to(device)

  def run(a, b):
    dv = lambda x: x[a:b].contiguous().to(device)
    return parity.cpu(net(dv(di['d']), dv(di['pts']), dv(di['rgb_feat']), dv(di['mask']), temb)).clone()

  return run(0, R), torch.cat([run(0, cut), run(cut, R)], 0)


def check_position_independence(device, S=64, R=5):
  """Nothing a ray's outputs are computed from depends on the wave or the workgroup the ray sits in: both networks, every output, bit for bit.
  The dynamic network: R rays in one call against 2 + (R - 2).  The static network: against 1 + (R - 1), and the first two rays against a call of those
  two alone.  Static rays are NOT compared through a call of exactly three rays: there the static branch reproduces the reference's `torch.cross`
  without `dim` (render_ray.py:375, :392 -- tests/golden/cross_axis.npz), which crosses over the rays instead of xyz, so a ray's
  Pluecker coordinates, and with them rgb and sigma, differ by design from the same ray in a chunk of another size (on the parent commit as well)."""
  whole, parts = dynamic_split_outputs(device, 'small', S, R, 2)
  parity.assert_bitexact(whole[..., :3], parts[..., :3], f'dynamic rgb, {R} rays in one call vs 2 + {R - 2}')
  parity.assert_bitexact(whole[..., 3], parts[..., 3], f'dynamic sigma, {R} rays in one call vs 2 + {R - 2}')
  assert R - 1 != 3 and R != 3
  whole, parts = static_split_outputs(device, 'small', S, R, 1)
  parity.assert_bitexact(whole[..., :3], parts[..., :3], f'static rgb, {R} rays in one call vs 1 + {R - 1}')
  parity.assert_bitexact(whole[..., 3], parts[..., 3], f'static sigma, {R} rays in one call vs 1 + {R - 1}')
  pair, one_one = static_split_outputs(device, 'small', S, 2, 1)
  parity.assert_bitexact(whole[:2], pair, f'static raw of rays 0-1, {R} rays in one call vs a call of the two')
  parity.assert_bitexact(pair, one_one, 'static raw of rays 0-1, one call vs 1 + 1')
