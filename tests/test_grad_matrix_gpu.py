"""orth_project's HIP backward against the float64 autograd reference (tests/grad_autograd_ref.py).

A covering matrix of reductions, value maps, depth channels, valid maps, to_global / flip_h, fills
and losses (MATRIX in tests/test_grad_ref_cpu.py), g15, and the branches the matrix does not reach:
partial needs_input_grad, per-frame argument shapes, the pitch clamp's edge, holes in the depth,
dtypes and strided inputs, CPU tensors, retain_graph and accumulation, the cfg3-like scale and a
batch whose backward grid-strides.

Bars: value gradients bit-exact; depth gradients within 1e-5 of the largest magnitude; camera
gradients within 1e-5 relative.  Gradients of the same call compared with each other are
bit-exact (value / depth) or within 1e-6 relative (camera: float64 atomics in any order)."""
import numpy as np
import pytest
import torch

from test_grad_cpu import assert_close_rel
from test_grad_ref_cpu import G15_NAMES, MATRIX, case_reference, g15_config, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEAVES = ("depth", "value", "pitch", "cam_height")
GRAD = {"depth": "grad_depth", "value": "grad_value", "pitch": "grad_pitch", "cam_height": "grad_cam_height"}


def run(a, kw, dev=DEV, wants=LEAVES, dtype=torch.float32, depth=None, value=None, retain=False):
  """One orth_project call with the case's loss backpropagated.  Returns (leaves dict, outputs)."""
  import dungeon_maps_amd as dmap
  t = lambda x, name, dt=torch.float32: torch.tensor(np.asarray(x), dtype=dt, device=dev).requires_grad_(
      name in wants)
  leaves = {"depth": t(a["depth"], "depth", dtype) if depth is None else depth,
            "value": (t(a["value"], "value", dtype) if value is None else value) if "value" in a else None,
            "pitch": t(kw["cam_pitch"], "pitch"), "cam_height": t(kw["cam_height"], "cam_height")}
  valid = torch.tensor(a["valid"], device=dev) if "valid" in a else None
  outs = dmap.orth_project(leaves["depth"], leaves["value"], valid,
                           **dict(kw, cam_pitch=leaves["pitch"], cam_height=leaves["cam_height"]))
  loss_of(a, outs).backward(retain_graph=retain)
  return leaves, outs


def loss_of(a, outs):
  """The case's loss; a loss on the height map alone leaves the topdown map out of the graph."""
  dev = outs[0].device
  terms = []
  if a["loss"] != "height":
    terms.append((torch.tensor(a["weights"], device=dev) * outs[0]).sum())
  if a["loss"] != "top":
    terms.append((torch.tensor(a["hweights"], device=dev) * outs[2]).sum())
  return sum(terms)


def grads_of(leaves):
  g = lambda k: None if leaves[k] is None or leaves[k].grad is None else leaves[k].grad.detach().cpu().numpy()
  return {"grad_depth": g("depth"), "grad_value": g("value"), "grad_pitch": g("pitch"),
          "grad_cam_height": g("cam_height")}


def check(got, want, what=""):
  if want.get("grad_value") is not None:
    np.testing.assert_array_equal(got["grad_value"], want["grad_value"], err_msg=f"{what} value")
  assert_close_rel(got["grad_depth"], want["grad_depth"], what=f"{what} depth")
  assert_close_rel(got["grad_pitch"], want["grad_pitch"], what=f"{what} pitch")
  assert_close_rel(got["grad_cam_height"], want["grad_cam_height"], what=f"{what} cam_height")


def same_call(got, want, what=""):
  """Two runs of one configuration: value / depth bit-exact, camera within 1e-6 relative."""
  for k in ("grad_value", "grad_depth"):
    if want.get(k) is not None:
      np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
  for k in ("grad_pitch", "grad_cam_height"):
    if want.get(k) is not None:
      assert_close_rel(got[k], want[k], rtol=1e-6, what=f"{what} {k}")


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MATRIX))
def test_backward_matches_autograd_reference(name):
  a, kw = make_case(name)
  leaves, outs = run(a, kw)
  check(grads_of(leaves), case_reference(a, kw), name)


@pytest.mark.parametrize("name", G15_NAMES)
def test_backward_matches_reference_g15(name):
  a, kw = g15_config(name)
  a = dict(a, loss="both" if a["loss_top"] and "hweights" in a else ("top" if a["loss_top"] else "height"))
  leaves, outs = run(a, kw)
  got = grads_of(leaves)
  if "grad_value" in a:
    np.testing.assert_array_equal(got["grad_value"], a["grad_value"])
  assert_close_rel(got["grad_depth"], a["grad_depth"], what="depth")
  assert got["grad_pitch"].shape == a["grad_pitch"].shape
  assert got["grad_cam_height"].shape == a["grad_cam_height"].shape
  assert_close_rel(got["grad_pitch"], a["grad_pitch"], what="pitch")
  assert_close_rel(got["grad_cam_height"], a["grad_cam_height"], what="cam_height")
  if name == "max_pitch_at_eps":
    assert got["grad_pitch"][0] == 0 and got["grad_pitch"][1] != 0


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["max_cont_dc3_local", "mean_h_dc1", "max_onehot_height", "sum_onehot_both"])
@pytest.mark.parametrize("only", LEAVES)
def test_gradients_of_a_subset_of_inputs_equal_the_full_runs(name, only):
  """needs_input_grad with one input: the others' gradients are None, the asked one is the full
  run's (the backward takes other branches: no moments for value alone, moments without a depth
  gradient for cam_height alone)."""
  a, kw = make_case(name)
  if only == "value" and "value" not in a:
    pytest.skip("no value map")
  full = grads_of(run(a, kw)[0])
  leaves, _ = run(a, kw, wants=(only,))
  got = grads_of(leaves)
  for k in LEAVES:
    if k != only:
      assert got[GRAD[k]] is None, k
  assert got[GRAD[only]] is not None
  if not (only == "value" and a["loss"] == "height"):       # (a loss on the height map alone: zeros)
    assert np.count_nonzero(full[GRAD[only]]) > 0
  same_call({GRAD[only]: got[GRAD[only]]}, {GRAD[only]: full[GRAD[only]]}, f"{name} {only}")


@pytest.mark.parametrize("shape", ["0d", "1", "B1", "float_pitch"])
def test_per_frame_arguments_of_one_row_or_a_column(shape):
  """A 0-d / (1,) cam_height / cam_pitch requiring grad is shared by the B frames: its gradient is
  the sum of the (B,) run's; (B, 1) keeps its shape; a python float pitch next to a tensor height."""
  a, kw = make_case("max_cont_dc3_local", B=3)
  B = 3
  kw = dict(kw, cam_pitch=np.full(B, kw["cam_pitch"][0]), cam_height=np.full(B, kw["cam_height"][0]))
  full = grads_of(run(a, kw)[0])
  if shape == "float_pitch":
    kw2 = dict(kw, cam_pitch=float(kw["cam_pitch"][0]))
    import dungeon_maps_amd as dmap
    depth = torch.tensor(a["depth"], device=DEV, requires_grad=True)
    h = torch.tensor(kw["cam_height"], device=DEV, requires_grad=True)
    outs = dmap.orth_project(depth, torch.tensor(a["value"], device=DEV), torch.tensor(a["valid"], device=DEV),
                             **dict(kw2, cam_height=h))
    loss_of(a, outs).backward()
    np.testing.assert_array_equal(depth.grad.cpu().numpy(), full["grad_depth"])
    assert_close_rel(h.grad.cpu().numpy(), full["grad_cam_height"], rtol=1e-6)
    return
  form = {"0d": lambda x: np.float32(x[0]), "1": lambda x: x[:1], "B1": lambda x: x.reshape(B, 1)}[shape]
  kw2 = dict(kw, cam_pitch=form(kw["cam_pitch"]), cam_height=form(kw["cam_height"]))
  leaves, _ = run(a, kw2)
  got = grads_of(leaves)
  np.testing.assert_array_equal(got["grad_depth"], full["grad_depth"])
  np.testing.assert_array_equal(got["grad_value"], full["grad_value"])
  for k in ("grad_pitch", "grad_cam_height"):
    want = full[k].sum() if shape in ("0d", "1") else full[k]
    assert got[k].shape == np.shape(kw2["cam_pitch"])
    assert_close_rel(got[k].reshape(-1), np.reshape(want, -1), rtol=1e-6, what=k)
  check(got, case_reference(a, kw2), shape)


def test_pitch_at_the_clamp_and_one_ulp_either_side():
  """|a| <= 1e-3f rotates by 0 (frames.py) and has no pitch gradient (_camera_grads): both sides
  must agree on the float32 boundary."""
  eps = np.float32(0.001)
  pitch = np.array([eps, np.nextafter(eps, np.float32(1)), np.nextafter(eps, np.float32(0)), -eps,
                    -np.nextafter(eps, np.float32(1))], dtype=np.float32)
  a, kw = make_case("max_h_dc1", B=5)
  kw = dict(kw, cam_pitch=pitch)
  got = grads_of(run(a, kw)[0])
  check(got, case_reference(a, kw), "pitch edge")
  assert got["grad_pitch"][0] == 0 and got["grad_pitch"][2] == 0 and got["grad_pitch"][3] == 0
  assert got["grad_pitch"][1] != 0 and got["grad_pitch"][4] != 0


@pytest.mark.parametrize("name", ["max_h_dc1", "mean_cont_both", "sum_h_dc3_local"])
def test_depth_holes_get_no_gradient(name):
  """Habitat-style holes (0, +inf, NaN) fall out under the truncation: their gradient is exactly 0
  and every gradient is finite (no invalid pixel reaches the moments)."""
  a, kw = make_case(name)
  rng = np.random.default_rng(3)
  d = a["depth"].copy()
  holes = rng.integers(0, 3, size=d.shape)
  hit = rng.uniform(size=d.shape) < 0.1
  d[hit & (holes == 0)] = 0.0
  d[hit & (holes == 1)] = np.inf
  d[hit & (holes == 2)] = np.nan
  a = dict(a, depth=d)
  got = grads_of(run(a, kw)[0])
  for k, g in got.items():
    assert g is None or np.isfinite(g).all(), k
  assert (got["grad_depth"][hit] == 0).all()
  check(got, case_reference(a, kw), name)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_half_and_double_inputs_get_the_float32_gradient_cast(dtype):
  a, kw = make_case("mean_cont_both")
  np_dt = {torch.float16: np.float16, torch.float64: np.float64}[dtype]
  a32 = dict(a, depth=a["depth"].astype(np_dt).astype(np.float32), value=a["value"].astype(np_dt).astype(np.float32))
  want = grads_of(run(a32, kw)[0])
  leaves, _ = run(a32, kw, dtype=dtype)
  assert leaves["depth"].grad.dtype == dtype and leaves["value"].grad.dtype == dtype
  got = grads_of(leaves)
  for k in ("grad_depth", "grad_value"):
    np.testing.assert_array_equal(got[k], want[k].astype(np_dt))


def test_strided_depth_and_value_views():
  """A channel slice of depth and a transposed value view go through .contiguous() under autograd."""
  a, kw = make_case("max_cont_dc3_local")
  B, dc, H, W = a["depth"].shape
  want = grads_of(run(a, kw)[0])
  wide = torch.tensor(np.concatenate([a["depth"], a["depth"]], 1), device=DEV, requires_grad=True)
  vt = torch.tensor(np.ascontiguousarray(a["value"].transpose(0, 1, 3, 2)), device=DEV, requires_grad=True)
  depth, value = wide[:, dc:], vt.transpose(2, 3)
  assert not depth.is_contiguous() and not value.is_contiguous()
  run(a, kw, depth=depth, value=value)
  np.testing.assert_array_equal(wide.grad[:, dc:].cpu().numpy(), want["grad_depth"])
  assert not wide.grad[:, :dc].any()
  np.testing.assert_array_equal(vt.grad.transpose(2, 3).cpu().numpy(), want["grad_value"])


def test_cpu_tensors_with_a_value_map():
  a, kw = make_case("min_cont_local")
  want = grads_of(run(a, kw)[0])
  leaves, outs = run(a, kw, dev="cpu")
  assert outs[0].device.type == "cpu" and leaves["depth"].grad.device.type == "cpu"
  same_call(grads_of(leaves), want, "cpu")


def test_backward_twice_with_retain_graph_and_accumulation_over_two_calls():
  a, kw = make_case("max_onehot_top")
  once = grads_of(run(a, kw)[0])
  leaves, outs = run(a, kw, retain=True)
  loss_of(a, outs).backward()
  twice = grads_of(leaves)
  same_call(twice, {k: 2 * v for k, v in once.items()}, "retain_graph")
  # two calls on the same leaves: the gradients add
  import dungeon_maps_amd as dmap
  b = dict(a, weights=np.flip(a["weights"], -1).copy(), hweights=np.flip(a["hweights"], -1).copy())
  other = grads_of(run(b, kw)[0])
  valid = torch.tensor(a["valid"], device=DEV)
  for lv in leaves.values():
    lv.grad = None
  call = lambda: dmap.orth_project(leaves["depth"], leaves["value"], valid,
                                   **dict(kw, cam_pitch=leaves["pitch"], cam_height=leaves["cam_height"]))
  loss_of(a, call()).backward()
  loss_of(b, call()).backward()
  same_call(grads_of(leaves), {k: once[k] + other[k] for k in once}, "two calls")


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("red,vkind", [("max", "onehot"), ("mean", "cont")])
def test_cfg3_like_scale(red, vkind):
  """40 value channels, 640x480 -> 512x512 (cfg3's geometry) at B=2, loss on both maps."""
  a, kw = make_case("max_onehot_top" if vkind == "onehot" else "mean_cont_both", H=480, W=640, mh=512, mw=512,
                    res=0.03, reduction=red, vc=40, loss="both", valid="none")
  leaves, _ = run(a, kw)
  got = grads_of(leaves)
  assert np.count_nonzero(got["grad_value"]) > 1000 and np.count_nonzero(got["grad_depth"]) > 1000
  check(got, case_reference(a, kw), "cfg3-like")


def test_many_frames_grid_stride():
  """B = 130 frames of 320x240: backward_blocks takes its floor of 16 workgroups per frame while a
  frame needs 300, so each thread loops ~19 times and 16 workgroups add into each frame's moments."""
  a, kw = make_case("max_h_dc1", B=130, H=240, W=320, mh=128, mw=128, res=0.05, valid="b1")
  leaves, _ = run(a, kw)
  got = grads_of(leaves)
  assert (got["grad_cam_height"] != 0).all()
  check(got, case_reference(a, kw), "B130")
