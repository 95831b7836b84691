"""The float64 autograd reference of orth_project's backward (tests/grad_autograd_ref.py) without a GPU.

* against the reference's own gradients, g14 and g15 (tests/golden/gen_golden_grad.py);
* against the numpy chain-rule helper (tests/grad_expect.py) on every configuration of the GPU
  matrix (tests/test_grad_matrix_gpu.py) -- two derivations, one by hand, one by autograd;
* torch.autograd.gradcheck of its differentiable piece with the cells and winners held fixed.

Bars: value gradients bit-exact, depth / camera gradients within 1e-5 relative."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from grad_autograd_ref import chain, prepare, reference_grads
from grad_expect import expected_grads
from test_grad_cpu import _NAMES as G14_NAMES, assert_close_rel, case_config

# ---------------------------------------------------------------------------------------------
# The configuration matrix.  Geometry: B frames of W x H -> a MH x MW map, a floor and walls
# seen by a pitched camera.
# name: reduction, value ('none' / 'onehot' / 'cont'), vc, dc, valid (None / 'b1' / 'bdc'),
#       to_global, flip_h, fill ('in' = inside the data range), loss ('top' / 'height' / 'both')
# ---------------------------------------------------------------------------------------------
MATRIX = {
    "max_h_dc1":            ("max", "none", 0, 1, None, True, True, -np.inf, "top"),
    "max_h_dc3_valid_b1":   ("max", "none", 0, 3, "b1", True, False, None, "both"),
    "max_h_fill_in":        ("max", "none", 0, 1, "bdc", False, True, "in", "top"),
    "min_h_dc3_valid_bdc":  ("min", "none", 0, 3, "bdc", True, True, np.inf, "top"),
    "min_h_fill_in":        ("min", "none", 0, 1, None, True, False, "in", "height"),
    "sum_h_dc3_local":      ("sum", "none", 0, 3, "b1", False, True, None, "top"),
    "mean_h_dc1":           ("mean", "none", 0, 1, "bdc", True, True, None, "top"),
    "mean_h_dc3_local":     ("mean", "none", 0, 3, None, False, False, -np.inf, "both"),
    "max_onehot_top":       ("max", "onehot", 4, 1, "b1", True, True, None, "top"),
    "max_onehot_height":    ("max", "onehot", 4, 1, None, False, True, None, "height"),
    "max_cont_dc3_local":   ("max", "cont", 3, 3, "bdc", False, False, -np.inf, "both"),
    "max_cont_dc2_fill_in": ("max", "cont", 2, 2, "b1", True, False, "in", "top"),
    "min_cont_local":       ("min", "cont", 3, 1, "b1", False, True, np.inf, "both"),
    "min_cont_fill_in":     ("min", "cont", 2, 1, None, True, True, "in", "both"),
    "sum_onehot_both":      ("sum", "onehot", 4, 1, "bdc", True, True, None, "both"),
    "sum_cont_dc3_height":  ("sum", "cont", 3, 3, "b1", False, True, None, "height"),
    "mean_cont_both":       ("mean", "cont", 3, 1, None, True, False, None, "both"),
    "mean_onehot_dc3":      ("mean", "onehot", 3, 3, "bdc", False, True, -np.inf, "top"),
    "mean_cont_dc2_height": ("mean", "cont", 2, 2, "bdc", True, True, -np.inf, "height"),
}
FILL_IN = {"none": 0.05, "onehot": 0.5, "cont": 1.0}      # floor heights ~0, walls up to ~1.4; values in [0, 2]


def scene(rng, B, dc, H, W, pitch, cam_h, fx):
  """Floor plane plus walls of random depth, (B, dc, H, W) float32."""
  r = np.arange(H, dtype=np.float64)[:, None]
  yn = ((H - 1) - r - H / 2.) / fx
  out = np.empty((B, dc, H, W), dtype=np.float32)
  for b in range(B):
    ky = np.cos(pitch[b]) * yn + np.sin(pitch[b])
    with np.errstate(divide="ignore"):
      floor = np.where(ky < -1e-6, -cam_h[b] / ky, 6.0) * np.ones((1, W))
    for c in range(dc):
      walls = np.full((H, W), 6.0)
      for _ in range(4):
        c0 = rng.integers(0, W - 8)
        walls[:, c0:c0 + rng.integers(4, W // 3)] = rng.uniform(1.0, 4.5)
      d = np.minimum(floor, walls) + rng.normal(0, 0.003, size=(H, W))
      out[b, c] = np.clip(d, 0.1, 6.0)
  return out


def make_case(name, B=2, H=60, W=80, mh=48, mw=48, res=0.12, seed=None, reduction=None, value=None, vc=None,
              dc=None, valid=None, to_global=None, flip_h=None, fill="same", loss=None):
  """(arrays, orth_project keyword arguments) of one matrix entry; keywords override it."""
  from oracle import oracle
  m = MATRIX[name]
  red = reduction or m[0]
  vkind = value or m[1]
  vc = m[2] if vc is None else vc
  dc = dc or m[3]
  valid = m[4] if valid is None else (None if valid == "none" else valid)
  to_global = m[5] if to_global is None else to_global
  flip_h = m[6] if flip_h is None else flip_h
  fill = m[7] if fill == "same" else fill
  fill = FILL_IN[vkind] if fill == "in" else fill
  loss = loss or m[8]
  rng = np.random.default_rng(seed if seed is not None else sum(map(ord, name)))
  cx, cy, fx, fy = oracle.camera_intrinsics(W, H, np.radians(70.))
  pitch = np.radians(rng.uniform(-25., -15., size=B)).astype(np.float32)
  cam_h = rng.uniform(0.8, 1.0, size=B).astype(np.float32)
  a = {"depth": scene(rng, B, dc, H, W, pitch, cam_h, fx), "pitch": pitch, "cam_height": cam_h}
  if vkind == "onehot":
    cls = rng.integers(0, vc, size=(B, 1, H, W))
    cls[:, :, :, : W // 3] = 1                            # a block of one class: ties in many cells
    a["value"] = (np.arange(vc)[None, :, None, None] == cls).astype(np.float32)
  elif vkind == "cont":
    a["value"] = rng.uniform(0.0, 2.0, size=(B, vc, H, W)).astype(np.float32)
  if valid:
    a["valid"] = rng.uniform(size=(B, 1 if valid == "b1" else dc, H, W)) > 0.15
  oc = vc or dc
  a["weights"] = rng.normal(size=(B, oc, mh, mw)).astype(np.float32)
  a["hweights"] = rng.normal(size=(B, oc, mh, mw)).astype(np.float32)
  a["loss"] = loss
  pose = np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-3, 3, B)], 1)
  kw = dict(cam_pose=pose.astype(np.float32), width_offset=mw / 2., height_offset=mh / 2., cam_pitch=pitch,
            cam_height=cam_h, map_res=res, map_width=mw, map_height=mh, focal_x=fx, focal_y=fy,
            center_x=cx, center_y=cy, trunc_depth_min=0.15, trunc_depth_max=5.05, trunc_height_max=None,
            clip_border=None, to_global=to_global, flip_h=flip_h, fill_value=fill, reduction=red,
            get_height_map=loss != "top" or bool(vc))
  return a, kw


def loss_weights(a):
  """(W_top, W_height) of the case's loss, as reference_grads takes them (None: term absent)."""
  return (a["weights"] if a["loss"] != "height" else np.zeros_like(a["weights"]),
          a["hweights"] if a["loss"] != "top" else None)


def case_reference(a, kw, **over):
  W_top, W_height = loss_weights(a)
  return reference_grads(a["depth"], dict(kw, **over), W_top=W_top, W_height=W_height,
                         value=a.get("value"), valid=a.get("valid"))


# ---------------------------------------------------------------------------------------------
def _check_against(want, got, what):
  if "grad_value" in want:
    np.testing.assert_array_equal(got["grad_value"], want["grad_value"], err_msg=f"{what}: value")
  assert_close_rel(got["grad_depth"], want["grad_depth"], what=f"{what}: depth")
  assert_close_rel(got["grad_pitch"], want["grad_pitch"], what=f"{what}: pitch")
  assert_close_rel(got["grad_cam_height"], want["grad_cam_height"], what=f"{what}: cam_height")


@pytest.mark.parametrize("name", G14_NAMES)
def test_autograd_reference_matches_reference_g14(name):
  a, kw = case_config(name)
  got = reference_grads(a["depth"], kw, W_top=a["weights"], W_height=a.get("hweights"),
                        value=a.get("value"), valid=a.get("valid"))
  _check_against(a, got, name)
  if name == "max_pitch_clamp":
    assert got["grad_pitch"][0] == 0


def _g15():
  arrays, cfg = load_golden("g15_orth_project_grad")
  return arrays, cfg, [str(c) for c in arrays["cases"]]


G15, G15_CFG, G15_NAMES = _g15()


def g15_config(name):
  """(arrays of one g15 case, orth_project keyword arguments of it).  cam_height / cam_pitch keep
  the shape the reference was called with (a 0-d cam_height is shared by both frames)."""
  from oracle import oracle
  a = {k.split("/", 1)[1]: v for k, v in G15.items() if k.startswith(name + "/")}
  c = {k[4:]: (v.item() if v.ndim == 0 else v) for k, v in a.items() if k.startswith("cfg_")}
  nan = lambda v: None if isinstance(v, float) and np.isnan(v) else v
  cx, cy, fx, fy = oracle.camera_intrinsics(G15_CFG["width"], G15_CFG["height"], G15_CFG["hfov"])
  kw = dict(cam_pose=a["cam_pose"], width_offset=G15_CFG["width_offset"], height_offset=G15_CFG["height_offset"],
            cam_pitch=a["pitch"], cam_height=a["cam_height"], map_res=G15_CFG["map_res"],
            map_width=G15_CFG["map_width"], map_height=G15_CFG["map_height"], focal_x=fx, focal_y=fy,
            center_x=cx, center_y=cy, trunc_depth_min=nan(c["dmin"]), trunc_depth_max=nan(c["dmax"]),
            trunc_height_max=nan(c["hmax"]), clip_border=c["clip"] or None, to_global=bool(c["to_global"]),
            flip_h=bool(c["flip_h"]), fill_value=None if c["fill_is_none"] else c["fill"],
            reduction=c["reduction"], get_height_map=bool(c["get_height"]))
  return a, kw


def g15_weights(a):
  """(W_top, W_height) of a g15 case; a case with loss_top == 0 has no topdown term."""
  return (a["weights"] if a["loss_top"] else None), a.get("hweights")


@pytest.mark.parametrize("name", G15_NAMES)
def test_autograd_reference_matches_reference_g15(name):
  a, kw = g15_config(name)
  W_top, W_height = g15_weights(a)
  got = reference_grads(a["depth"], kw, W_top=np.zeros_like(a["weights"]) if W_top is None else W_top,
                        W_height=W_height, value=a.get("value"), valid=a.get("valid"))
  _check_against(a, got, name)
  assert got["grad_pitch"].shape == a["grad_pitch"].shape
  assert got["grad_cam_height"].shape == a["grad_cam_height"].shape
  if name == "max_pitch_at_eps":
    assert a["grad_pitch"][0] == 0 and got["grad_pitch"][0] == 0     # |a| == 1e-3f: clamped
    assert a["grad_pitch"][1] != 0 and got["grad_pitch"][1] != 0     # one ulp above: live


def test_g15_cases_reach_what_they_are_named_for():
  a, kw = g15_config("max_height_fill_in_range")
  fill = np.float32(kw["fill_value"])
  assert (a["topdown"] == fill).any() and (a["topdown"] > fill).any() and not a["mask"][a["topdown"] == fill].any()
  a, _ = g15_config("max_pitch_at_eps")
  assert a["pitch"][0] == np.float32(0.001) and a["pitch"][1] == np.nextafter(np.float32(0.001), np.float32(1))
  a, _ = g15_config("height_only_loss_onehot")
  assert not a["loss_top"] and np.count_nonzero(a["grad_depth"]) and not np.count_nonzero(a["grad_value"])
  a, _ = g15_config("max_onehot_shared_cam_height")
  assert a["cam_height"].shape == () and a["grad_cam_height"].shape == ()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MATRIX))
def test_autograd_reference_matches_chain_rule_helper(name):
  from oracle import oracle
  a, kw = make_case(name)
  okw = {k: v for k, v in kw.items() if k != "get_height_map"}
  res = oracle.orth_project(a["depth"], value_map=a.get("value"), valid_map=a.get("valid"), debug=True,
                            **okw)
  W_top, W_height = loss_weights(a)
  vc = "value" in a
  H, W = a["depth"].shape[2:]
  g_depth, g_value, g_pitch, g_h = expected_grads(
      res[-1], a["depth"], res[0], res[1], W_top=W_top + (W_height if (W_height is not None and not vc) else 0),
      W_height=W_height if vc else None, value=a.get("value"), reduction=kw["reduction"], pitch=kw["cam_pitch"],
      H=H, W=W, cx=kw["center_x"], cy=kw["center_y"], fx=kw["focal_x"], fy=kw["focal_y"], flip_h=kw["flip_h"],
      mh=kw["map_height"], mw=kw["map_width"])
  want = {"grad_depth": g_depth, "grad_pitch": g_pitch, "grad_cam_height": g_h}
  if vc:
    want["grad_value"] = g_value
  got = case_reference(a, kw)
  _check_against(want, got, name)
  assert np.count_nonzero(got["grad_depth"]) > 0 or (vc and a["loss"] == "top")


def test_matrix_cases_reach_what_they_are_named_for():
  """The in-range fills leave cells at the fill next to cells past it; the scenes hit the maps."""
  from oracle import oracle
  for name, m in MATRIX.items():
    a, kw = make_case(name)
    okw = {k: v for k, v in kw.items() if k != "get_height_map"}
    top, mask = oracle.orth_project(a["depth"], value_map=a.get("value"), valid_map=a.get("valid"), **okw)[:2]
    if m[0] in ("sum", "mean") and m[7] in (np.inf, -np.inf):
      assert not mask.any(), name       # fill + x == fill: no cell changes (the gradients still flow)
    elif m[7] != "in":
      assert mask.mean() > 0.05, name
    else:
      fill = kw["fill_value"]
      past = top > fill if m[0] == "max" else top < fill
      assert past.any() and (top == fill).any() and not mask[top == fill].any(), name


@pytest.mark.parametrize("name", ["max_h_dc1", "mean_cont_both", "max_cont_dc3_local", "sum_h_dc3_local"])
def test_autograd_reference_chain_passes_gradcheck(name):
  """The restated chain is itself a correct derivative: float64 gradcheck with cells and winners
  fixed (a small crop of frames so the Jacobian stays cheap)."""
  a, kw = make_case(name, H=12, W=16, mh=12, mw=12, res=0.5)
  fixed = prepare(a["depth"], kw, value=a.get("value"), valid=a.get("valid"))
  B, dc = a["depth"].shape[:2]
  f64 = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64).requires_grad_()
  d, p, h = f64(a["depth"].reshape(B, dc, -1)), f64(kw["cam_pitch"]), f64(kw["cam_height"])
  v = f64(a["value"].reshape(B, a["value"].shape[1], -1)) if "value" in a else None
  if v is None:
    fn = lambda d, p, h: chain(fixed, d, None, p, h)[0]
    inputs = (d, p, h)
  else:
    fn = lambda d, v, p, h: tuple(x for x in chain(fixed, d, v, p, h) if x is not None)
    inputs = (d, v, p, h)
  assert fixed["top"].get("win_cell", fixed["top"].get("cell")).numel() > 0
  assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-7, rtol=1e-5)
