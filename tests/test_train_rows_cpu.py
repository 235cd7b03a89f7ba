"""The yardstick of tests/train_rows.py, checked without running a kernel: the exact family's preconditions hold at every shape, each float64
restatement agrees with autograd through the oracle (or torch.nn.functional), and the fp32 restatement family (b) takes its limit from does err."""
import pytest
import torch
import torch.nn.functional as F

import train_rows as T
from oracle import ibr_oracle as O


@pytest.fixture()
def dry():
  T.DRY[0] = True
  T.DRY_ERR32.clear()
  yield 'cpu'
  T.DRY[0] = False


@pytest.mark.parametrize('name', sorted(T.GROUPS))
def test_references_and_exact_preconditions_at_every_shape(dry, name):
  """every case of every group builds its inputs and float64 references; `_exact` / `_sum_exact` assert that the result is an fp32 number and that
  no partial sum can round (sum |terms| / lsb < 2^24) -- on the reference alone"""
  T.run_group(dry, name)


def test_exact_preconditions_of_the_tall_case(dry):
  T.check_act_bwd_tall(dry)


def test_fp32_restatements_err_where_the_limit_relies_on_them(dry):
  """family (b)'s limit is twice the fp32 restatement's own error: that error must not vanish (the limit would fall back to the 2e-6 floor alone
  without anyone noticing) for any output that goes through a transcendental or a division"""
  for name in ('view_weights', 'layernorm', 'blend', 'dynamic_head', 'embed', 'dynamic_embed', 'static_embed', 'vis_split', 'vis_split_act_bwd-plain', 'vis_split_act_bwd-fused'):
    T.run_group(dry, name)
  assert len(T.DRY_ERR32) >= 20
  zero = [k for k, e in T.DRY_ERR32.items() if e == 0.0]
  assert not zero, f'fp32 restatements without error: {zero}'
  assert max(T.DRY_ERR32.values()) < 1e-2  # ...and they are restatements of the same formula, not of another one


def test_precondition_helpers_reject_what_they_should():
  with pytest.raises(AssertionError):
    T._exact(torch.tensor([1.0 / 3.0], dtype=torch.float64), 'third')
  with pytest.raises(AssertionError):
    T._sum_exact(torch.tensor([[2.0 ** 19, 1.0 / 64]], dtype=torch.float64), 1, 'needs 26 bits')
  assert T._lsb(torch.tensor([0.375, 2.0, 0.0])) == 0.125
  assert float(T._sum_exact(torch.tensor([[2.0 ** 19, 1.0 / 16]], dtype=torch.float64), 1, 'fits in 24 bits')) == 2.0 ** 19 + 1.0 / 16


def test_activation_derivative_from_the_saved_output():
  g = T.gen(3)
  z = torch.randn(400, generator=g).double()
  z[:3] = torch.tensor([0.0, -1e-9, 1e-9])
  for act, fn in ((1, F.elu), (2, F.relu)):
    zz = z.clone().requires_grad_(True)
    y = fn(zz)
    y.sum().backward()
    assert torch.allclose(T.dact(y.detach(), act), zz.grad, rtol=0, atol=1e-15)
  dY, Y = T.act_bwd_inputs(12, 5, 0)
  zz = torch.where(Y > 0, Y, torch.log1p(Y.clamp(min=-0.999))).requires_grad_(True)  # a pre-activation whose ELU is Y (Y > -1)
  keep = Y > -1
  (F.elu(zz) * dY).sum().backward()
  ref, _ = T.act_bwd_reference(dY, Y, 1, 0)
  assert torch.allclose(ref[keep], zz.grad[keep], rtol=1e-12, atol=1e-12)


def test_layernorm_restatement_against_torch():
  a, b, gamma, beta, dout = T.layernorm_inputs(9, 0)
  y = (a + b).requires_grad_(True)
  out, xhat, rstd = T.layernorm_restatement(y, gamma, beta)
  out.backward(dout)
  y2, g2, b2 = (a + b).requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
  ref = F.layer_norm(y2, (128,), g2, b2, 1e-6)
  ref.backward(dout)
  assert torch.allclose(out, ref, rtol=1e-12, atol=1e-12) and torch.allclose(y.grad, y2.grad, rtol=1e-10, atol=1e-12)
  assert torch.allclose((dout * xhat).sum(0), g2.grad, rtol=1e-10, atol=1e-12) and torch.allclose(dout.sum(0), b2.grad, rtol=1e-12, atol=1e-12)


def test_pooling_weight_restatements_against_the_oracle_formulas():
  """the oracle's static_net states the same lines over [R, S, V, 1] tensors"""
  dot, logit, mask, _, _, _ = T.view_weights_inputs(7, 5, 0)
  s = torch.tensor(-0.75, dtype=torch.float64)
  e = torch.exp(torch.abs(s) * (dot[None, :, :, None] - 1))
  m4 = mask[None, :, :, None]
  w = (e - torch.min(e, dim=2, keepdim=True)[0]) * m4
  w = w / (torch.sum(w, dim=2, keepdim=True) + 1e-8)
  assert torch.equal(T.view_weights0_restatement(dot, mask, s), w[0, :, :, 0])
  assert torch.equal(T.view_weights0_restatement(dot, mask, None), (m4 / (torch.sum(m4, dim=2, keepdim=True) + 1e-8))[0, :, :, 0])
  vis = torch.sigmoid(logit[None, :, :, None]) * m4
  w = vis / (torch.sum(vis, dim=2, keepdim=True) + 1e-8)
  got = T.view_weights1_restatement(logit, mask)
  assert torch.equal(got[0], vis[0, :, :, 0]) and torch.equal(got[1], w[0, :, :, 0])
  assert torch.equal(got[2], w.mean(dim=2)[0, :, 0]) and torch.equal(got[3], torch.sum(m4, dim=2)[0, :, 0])
  # the sign convention of d|s|/ds that the kernel must follow
  for sv, sign in ((0.75, 1.0), (-0.75, -1.0), (0.0, 0.0)):
    t = torch.tensor(sv, dtype=torch.float64, requires_grad=True)
    torch.abs(t).backward()
    assert float(t.grad) == sign


def test_meanvar_reference_is_the_oracles_function():
  x, w, *_ = T.meanvar_inputs(3, 5, 7, 0)
  mean, var = T.meanvar_reference(x, w)
  m2 = (x * w[:, :, None]).sum(1)
  assert torch.equal(mean, m2) and torch.equal(var, (w[:, :, None] * (x - m2[:, None]) ** 2).sum(1))


def test_blend_and_head_restatements_against_the_oracle_formulas():
  g = T.gen(1)
  P, V = 6, 4
  mask, nvalid = T.head_inputs(P, V, 0)
  logit, rgb, sigma = torch.randn(P, V, generator=g).double(), torch.rand(P, V, 3, generator=g).double(), torch.randn(P, generator=g).double()
  blend, raw = T.blend_restatement(logit, mask, rgb, sigma, nvalid)
  x = logit[None, :, :, None].masked_fill(mask[None, :, :, None] == 0, -1e9)
  b = F.softmax(x, dim=2)
  assert torch.equal(blend, b[0, :, :, 0]) and torch.allclose(raw[:, :3], torch.sum(rgb[None] * b, dim=2)[0], rtol=0, atol=1e-15)
  assert float(blend[0].sum()) == pytest.approx(1.0) and bool((blend[0] == 1.0 / V).all())  # a fully masked point blends uniformly
  assert bool((raw[nvalid < 1, 3] == -1e9).all()) and torch.equal(raw[nvalid >= 1, 3], sigma[nvalid >= 1])
  lg = torch.randn(P, 3, generator=g).double()
  raw = T.dynamic_head_restatement(lg, sigma, nvalid, 5.0)
  m3 = mask[None, :, :, None]
  rgb_ref = torch.sigmoid(lg[None]).masked_fill(torch.sum(m3.repeat(1, 1, 1, 3), 2) == 0, 0)
  assert torch.equal(raw[:, :3], rgb_ref[0]) and torch.equal(raw[:, 3], (sigma - 5.0).masked_fill(nvalid < 1, -1e9))


def test_embed_restatements_against_the_oracle():
  x = torch.randn(5, 3, generator=T.gen(2)).double()
  assert torch.equal(T.embed_restatement(x, T.OCTAVES5), O.periodic_embed(x, 5, 5, False))
  ref = O.periodic_embed(x, 16, 16, True)  # (the oracle's frequencies are fp32 numbers: so are the kernel's)
  assert torch.allclose(T.embed_restatement(x, T.MOTION_FREQS), ref, rtol=0, atol=1e-12)
  d = torch.randn(4, 3, generator=T.gen(3)).double()
  pe, de = T.dynamic_embed_restatement(x, d)
  assert pe.shape == (5, 33) and de.shape == (4, 27) and torch.equal(de[:, :3], F.normalize(d, dim=-1))


def test_static_embed_restatement_against_the_oracle_plucker_functions():
  """V = 3: torch.cross without dim runs over the views, as the reference does (tests/golden/cross_axis.npz pins the oracle)"""
  g = T.gen(4)
  for R, S, V in ((2, 5, 3), (4, 2, 8)):
    pts, centers = torch.randn(R, S, 3, generator=g).double(), torch.randn(V, 3, generator=g).double()
    ray_o, ray_d = torch.randn(R, 3, generator=g).double(), torch.randn(R, 3, generator=g).double()
    rd, feat, mask = torch.randn(R, S, V, 4, generator=g).double(), torch.rand(R, S, V, 35, generator=g).double(), torch.ones(R, S, V).double()
    a0, ref_pe, meff = T.static_embed_restatement(pts, ray_o, ray_d, centers, rd, feat, mask, True)
    ray = F.normalize(pts[:, :, None] - centers[None, None], dim=-1)                        # [R, S, V, 3]
    o = centers[None, None].expand(R, S, V, 3)
    mom = torch.linalg.cross(o, ray, dim=2 if V == 3 else 3)
    src = torch.cat([ray, mom], -1)
    assert torch.allclose(a0.view(R, S, V, 103)[..., 33:39], src, rtol=0, atol=1e-14)
    assert torch.equal(a0.view(R, S, V, 103)[..., :3], pts[:, :, None].expand(-1, -1, V, -1)) and torch.equal(a0[:, 99:], rd.reshape(-1, 4))
    dn = F.normalize(ray_d, dim=-1)
    assert torch.allclose(ref_pe[:, :6], torch.cat([dn, torch.linalg.cross(ray_o, dn, dim=-1)], -1), rtol=0, atol=1e-14)
    assert bool((meff == 1).all())


def test_every_row_entry_point_of_the_header_has_a_check():
  """every dyn_train_* export except the GEMM, the attention and the compositing backward kernels (tests of their own in tests/parity.py) is
  called by tests/train_rows.py"""
  import os
  import re
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  names = set(re.findall(r'\b(dyn_train_\w+)\s*\(', open(os.path.join(root, 'include', 'dynibar_hip.h')).read()))
  names = {n for n in names if not re.match(r'dyn_train_(gemm|attn|composite|objective|distloss)', n)}
  src = open(os.path.join(root, 'tests', 'train_rows.py')).read()
  called = set(re.findall(r"call\('(dyn_train_\w+)'", src))
  assert names and not (names - called), f'no direct check calls {sorted(names - called)}'
