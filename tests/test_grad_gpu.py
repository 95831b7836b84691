"""orth_project's autograd path on the GPU (HIP backward kernels, dm_backward.hip).

Against the reference's own gradients (g14: value gradients bit-exact, depth / camera gradients
within 1e-5 relative), against the oracle-fed numpy helper up to the cfg2 geometry, and the
properties of the path: forward outputs bit-equal to the no-grad call, no grad_fn without grad,
repeatable value / depth gradients, depth -> MapProjector -> crop_topdown_map -> loss."""
import numpy as np
import pytest
import torch

from grad_expect import expected_grads
from test_grad_cpu import _NAMES, assert_close_rel, case_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(a, kw, dev=DEV, grads=True):
  import dungeon_maps_amd as dmap
  t = lambda x, rg: torch.tensor(x, device=dev).requires_grad_(rg and grads)
  depth = t(a["depth"], True)
  value = t(a["value"], True) if "value" in a else None
  valid = torch.tensor(a["valid"], device=dev) if "valid" in a else None
  pitch, cam_h = t(a["pitch"], True), t(a["cam_height"], True)
  k = dict(kw, cam_pitch=pitch, cam_height=cam_h)
  outs = dmap.orth_project(depth, value, valid, **k)
  return (depth, value, pitch, cam_h), outs


def _loss(a, outs):
  loss = (torch.tensor(a["weights"], device=outs[0].device) * outs[0]).sum()
  if "hweights" in a:
    loss = loss + (torch.tensor(a["hweights"], device=outs[0].device) * outs[2]).sum()
  return loss


@pytest.mark.parametrize("name", _NAMES)
def test_backward_matches_reference_g14(name):
  a, kw = case_config(name)
  (depth, value, pitch, cam_h), outs = _run(a, kw)
  assert outs[0].grad_fn is not None and outs[0].requires_grad
  assert not outs[1].requires_grad                                     # mask: not differentiable
  _loss(a, outs).backward()
  if value is not None:
    np.testing.assert_array_equal(value.grad.cpu().numpy(), a["grad_value"])
  assert_close_rel(depth.grad.cpu().numpy(), a["grad_depth"], what="depth")
  assert_close_rel(pitch.grad.cpu().numpy(), a["grad_pitch"], what="pitch")
  assert_close_rel(cam_h.grad.cpu().numpy(), a["grad_cam_height"], what="cam_height")


def _scene(rng, B, H, W, dc=1):
  r = np.arange(H)[:, None]
  base = np.where(r > H * 0.45, 0.88 / np.maximum(np.sin(np.radians(20.)) + (r - H / 2) / (0.9 * W), 0.05), 6.0)
  d = np.broadcast_to(base, (B, dc, H, W)) + rng.uniform(0.0, 0.05, size=(B, dc, H, W))
  return np.clip(d, 0.1, 6.0).astype(np.float32)


# B, H, W, mh, mw, reduction, value channels, depth channels, fill
RANDOM = [
    (64, 480, 640, 512, 512, "max", 0, 1, -np.inf),                 # cfg2 geometry
    (4, 480, 640, 512, 512, "mean", 0, 1, None),
    (3, 120, 160, 96, 128, "min", 3, 3, np.inf),
    (2, 240, 320, 256, 256, "sum", 4, 1, None),
    (2, 96, 128, 64, 60, "max", 5, 1, None),                        # odd-width map, one-hot values
]


@pytest.mark.parametrize("cfg", RANDOM, ids=lambda c: f"B{c[0]}_{c[2]}x{c[1]}_{c[5]}_vc{c[6]}")
def test_backward_matches_oracle_fed_helper(cfg):
  from oracle import oracle
  B, H, W, mh, mw, red, vc, dc, fill = cfg
  rng = np.random.default_rng(B * 1000 + vc)
  cx, cy, fx, fy = oracle.camera_intrinsics(W, H, np.radians(70.))
  a = {"depth": _scene(rng, B, H, W, dc),
       "pitch": np.radians(rng.uniform(-25., -15., size=B)).astype(np.float32),
       "cam_height": rng.uniform(0.8, 1.0, size=B).astype(np.float32)}
  pose = np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-3, 3, B)], 1).astype(np.float32)
  if vc:
    if red == "max" and dc == 1:
      a["value"] = (np.arange(vc)[None, :, None, None] == rng.integers(0, vc, (B, 1, H, W))).astype(np.float32)
    else:
      a["value"] = rng.uniform(0, 2, (B, vc, H, W)).astype(np.float32)
    a["valid"] = rng.uniform(size=(B, 1, H, W)) > 0.1
  oc = vc or dc
  a["weights"] = rng.normal(size=(B, oc, mh, mw)).astype(np.float32)
  if vc:
    a["hweights"] = rng.normal(size=(B, oc, mh, mw)).astype(np.float32)
  kw = dict(cam_pose=pose, width_offset=mw / 2., height_offset=mh / 2., map_res=0.03 * 512 / mh,
            map_width=mw, map_height=mh, focal_x=fx, focal_y=fy, center_x=cx, center_y=cy,
            trunc_depth_min=0.15, trunc_depth_max=5.05, trunc_height_max=None, clip_border=None,
            to_global=True, flip_h=True, fill_value=fill, reduction=red, get_height_map=bool(vc))
  (depth, value, pitch, cam_h), outs = _run(a, kw)
  _loss(a, outs).backward()
  okw = {k: v for k, v in kw.items() if k != "get_height_map"}
  okw.update(cam_pitch=a["pitch"], cam_height=a["cam_height"])
  res = oracle.orth_project(a["depth"], value_map=a.get("value"), valid_map=a.get("valid"), debug=True,
                            nthreads=8, **okw)
  top, mask = outs[0].detach().cpu().numpy(), outs[1].cpu().numpy()
  np.testing.assert_array_equal(mask, res[1])
  g_depth, g_value, g_pitch, g_h = expected_grads(
      res[-1], a["depth"], top, mask, W_top=a["weights"], W_height=a.get("hweights"), value=a.get("value"),
      reduction=red, pitch=a["pitch"], H=H, W=W, cx=cx, cy=cy, fx=fx, fy=fy, flip_h=True, mh=mh, mw=mw)
  if vc:
    np.testing.assert_array_equal(value.grad.cpu().numpy(), g_value)
  assert_close_rel(depth.grad.cpu().numpy(), g_depth, what="depth")
  assert_close_rel(pitch.grad.cpu().numpy(), g_pitch, what="pitch")
  assert_close_rel(cam_h.grad.cpu().numpy(), g_h, what="cam_height")


@pytest.mark.parametrize("name", ["max_height", "max_onehot", "max_cont", "min_cont", "mean_cont", "sum_onehot"])
def test_grad_path_forward_equals_no_grad_path_and_no_grad_calls_have_no_grad_fn(name):
  a, kw = case_config(name)
  _, outs = _run(a, kw)
  _, plain = _run(a, kw, grads=False)
  with torch.no_grad():
    _, under = _run(a, kw)
  assert outs[0].grad_fn is not None
  exact = kw["reduction"] in ("max", "min")
  for o, p, u in zip(outs, plain, under):
    assert p.grad_fn is None and u.grad_fn is None and not p.requires_grad and not u.requires_grad
    for other in (p, u):
      if exact or o.dtype == torch.bool:
        np.testing.assert_array_equal(o.detach().cpu().numpy(), other.cpu().numpy())
      else:
        # sum / mean accumulate with float atomics: two no-grad calls differ in the last bits too
        np.testing.assert_allclose(o.detach().cpu().numpy(), other.cpu().numpy(), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("name", ["max_onehot", "mean_cont", "max_height"])
def test_value_and_depth_gradients_repeat_bit_for_bit(name):
  a, kw = case_config(name)
  got = []
  for _ in range(2):
    (depth, value, _, _), outs = _run(a, kw)
    _loss(a, outs).backward()
    got.append((depth.grad.cpu().numpy(), None if value is None else value.grad.cpu().numpy()))
  np.testing.assert_array_equal(got[0][0], got[1][0])
  if got[0][1] is not None:
    np.testing.assert_array_equal(got[0][1], got[1][1])


def test_cpu_tensors_and_the_height_map_twice():
  """CPU inputs go through the GPU and back with their gradient; without a value map the height map
  is the topdown map itself and the gradients of both uses add."""
  a, kw = case_config("max_height")
  (d1, _, _, _), outs = _run(a, dict(kw, get_height_map=True), dev="cpu")
  assert outs[0].device.type == "cpu" and outs[2] is outs[0]
  w = torch.tensor(a["weights"])
  ((w * outs[0]).sum() + (w * outs[2]).sum()).backward()
  assert_close_rel(d1.grad.numpy(), 2 * a["grad_depth"], what="depth twice")


def test_depth_through_projector_and_bilinear_crop():
  import dungeon_maps_amd as dmap
  from dungeon_maps_amd import utils
  rng = np.random.default_rng(5)
  B, H, W = 2, 48, 64
  proj = dmap.MapProjector(width=W, height=H, hfov=np.radians(70.), cam_pitch=np.radians(-20.), cam_height=0.88,
                           width_offset=32., height_offset=32., map_res=0.1, map_width=64, map_height=64,
                           trunc_depth_min=0.15, trunc_depth_max=5.05, to_global=True, fill_value=-np.inf)
  depth = torch.tensor(_scene(rng, B, H, W), device=DEV, requires_grad=True)
  pose = torch.tensor([[0.1, -0.1, 0.3], [0.0, 0.2, -0.4]])
  top, mask, height = proj.orth_project(depth, cam_pose=pose, get_height_map=True)
  assert top.grad_fn is not None
  tmap = dmap.TopdownMap(topdown_map=top, mask=mask, height_map=height, map_projector=proj)
  assert mask.any(), "no cell hit: the scene does not reach the map"
  center = torch.tensor([[32.3, 31.6], [31.4, 32.7]])        # most of the map, at fractional offsets
  crop = dmap.crop_topdown_map(tmap, center, 56, 52, mode="bilinear")
  wts = torch.tensor(rng.normal(size=tuple(crop.topdown_map.shape)).astype(np.float32), device=DEV)
  finite = torch.isfinite(crop.topdown_map.detach())                 # (unhit cells hold -inf)
  assert finite.any()
  loss = lambda c: torch.where(finite, wts * c, torch.zeros_like(c)).sum()
  g_top, = torch.autograd.grad(loss(crop.topdown_map), top, retain_graph=True)
  loss(crop.topdown_map).backward()
  g = depth.grad.cpu().numpy()
  assert np.isfinite(g).all() and np.count_nonzero(g) > 0
  # the crop's gradient is the torch route's (generate_crop_grid + image_sample)
  leaf = top.detach().requires_grad_()
  grid = utils.generate_crop_grid(center.to(DEV), 64, 64, 56, 52)
  ref = utils.image_sample(leaf, grid, fill_value=float("-inf"), mode="bilinear")
  g_ref, = torch.autograd.grad(loss(ref), leaf)
  # (grid_sample's backward accumulates with atomics on the GPU: equal up to the summation order)
  np.testing.assert_allclose(g_top.cpu().numpy(), g_ref.cpu().numpy(), rtol=1e-6, atol=1e-6)
