"""orth_project(label_map=, num_classes=) on the GPU: the label call returns, bit for bit, what the
same call returns with value_map[b, c] = (label_map[b, 0] == c) -- against the reference's recorded
fixtures, the oracle, and this library's own one-hot call over a matrix of reductions, fills, label
dtypes and geometries -- and the debug hook proves which route (native class-set kernels /
compatibility expansion) computed it.  Comparisons are assert_array_equal (NaNs in place are equal)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, project_kwargs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NATIVE, COMPAT = 1, 2


@pytest.fixture(scope="module")
def dmap():
  import dungeon_maps_amd as dmap
  from dungeon_maps_amd import _native
  _native.lib()
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU (run with -m gpu on an MI355X box)")
  return dmap


def _route():
  from dungeon_maps_amd import _native
  return _native.lib().dm_debug_last_label_route()


def _limit():
  from dungeon_maps_amd import _native
  return _native.LABEL_NATIVE_MAX_CLASSES


def _one_hot(labels, C):
  """The definition: value[b, c, y, x] = 1.0 if labels[b, 0, y, x] == c else 0.0."""
  lab = np.asarray(labels).astype(np.int64).reshape(labels.shape[0], 1, *labels.shape[-2:])
  return (lab == np.arange(C, dtype=np.int64).reshape(1, C, 1, 1)).astype(np.float32)


def _np(outs):
  torch.cuda.synchronize()
  return [o.cpu().numpy() for o in outs]


def _label_call(dmap, cfg, depth, labels, C, valid=None, **call):
  proj = dmap.MapProjector(**cfg)
  outs = proj.orth_project(
      torch.from_numpy(depth).to(DEV), label_map=torch.from_numpy(labels).to(DEV), num_classes=C,
      valid_map=None if valid is None else torch.from_numpy(valid).to(DEV), get_height_map=True, **call)
  return _np(outs), _route()


def _one_hot_call(dmap, cfg, depth, value, valid=None, **call):
  proj = dmap.MapProjector(**cfg)
  return _np(proj.orth_project(
      torch.from_numpy(depth).to(DEV), value_map=torch.from_numpy(value).to(DEV),
      valid_map=None if valid is None else torch.from_numpy(valid).to(DEV), get_height_map=True, **call))


def _assert_same(got, want, what=""):
  for g, w, name in zip(got, want, ("topdown", "mask", "height")):
    assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
    np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")


# ---- 1. pinned to the reference ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["g3_semantic_onehot5_64x48", "g3b_semantic_validmap_64x48"])
@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_fixture_one_hot_maps_from_their_labels(dmap, name, dtype):
  g, cfg = load_golden(name)
  value = g["value"]
  assert set(np.unique(value)) == {0.0, 1.0} and (value.sum(0) == 1).all()     # strict one-hot
  labels = value.argmax(0).astype(dtype)[None]
  valid = g["valid_map"] if "valid_map" in g else None
  got, route = _label_call(dmap, cfg, g["depth"], labels, value.shape[0], valid=valid)
  assert route == NATIVE
  _assert_same(got, (g["topdown"], g["mask"], g["height"]), name)


def test_builder_steps_with_labels_reproduce_the_reference_sequence(dmap):
  """The reference's object-map loop with its three one-hot lines dropped (fixture g5, semantic)."""
  g, cfg = load_golden("g5_builder_merge4_semantic")
  proj = dmap.MapProjector(**cfg)
  proj = proj.clone(fill_value=0.)
  proj.fill_value = 0.
  build = dmap.MapBuilder(map_projector=proj)
  build.reset()
  for t in range(4):
    value = g[f"value{t}"]
    assert set(np.unique(value)) == {0.0, 1.0} and (value.sum(0) == 1).all()
    seg = value.argmax(0).astype(np.int64)[..., None]              # (h, w, 1) int64, as a simulator gives it
    local = build.step(
        depth_map=torch.from_numpy(g[f"depth{t}"]).to(DEV), label_map=seg, num_classes=value.shape[0],
        cam_pose=g["poses"][t].copy(), to_global=False, map_res=0.05, width_offset=32.,
        height_offset=0., map_width=64, map_height=64, center_mode=dmap.CenterMode.none, merge=True)
    assert _route() == NATIVE
    wm = build.world_map
    np.testing.assert_array_equal(local.topdown_map.cpu().numpy(), g[f"local_map{t}"])
    np.testing.assert_array_equal(local.mask.cpu().numpy(), g[f"local_mask{t}"])
    np.testing.assert_array_equal(local.height_map.cpu().numpy(), g[f"local_height{t}"])
    assert [wm.proj.map_width, wm.proj.map_height] == g[f"world_size{t}"].tolist()
    np.testing.assert_array_equal(np.asarray(wm.proj.width_offset, dtype=np.float32), g[f"world_woff{t}"])
    np.testing.assert_array_equal(np.asarray(wm.proj.height_offset, dtype=np.float32), g[f"world_hoff{t}"])
    np.testing.assert_array_equal(wm.mask.cpu().numpy(), g[f"world_mask{t}"])
    np.testing.assert_array_equal(wm.topdown_map.cpu().numpy(), g[f"world_map{t}"])
    np.testing.assert_array_equal(wm.height_map.cpu().numpy(), g[f"world_height{t}"])


# ---- 2. / 7. the 40-class geometry: label call == one-hot call == oracle, and no state leaks -----
def _synthetic(B, H, W, seed):
  g = torch.Generator().manual_seed(seed)
  depth = torch.empty(B, 1, H, W).uniform_(0.1, 10.0, generator=g)
  pose = torch.empty(B, 3).uniform_(-1, 1, generator=g)
  pose[:, 2] = torch.empty(B).uniform_(-np.pi, np.pi, generator=g)
  return depth.numpy(), pose.numpy()


def test_semantic_40_classes_labels_vs_one_hot_vs_oracle(dmap, oracle):
  B, H, W, C = 2, 120, 160, 40
  depth, pose = _synthetic(B, H, W, seed=99)
  g = torch.Generator().manual_seed(5)
  labels = torch.randint(0, C, (B, H, W), generator=g)
  value = torch.nn.functional.one_hot(labels, C).permute(0, 3, 1, 2).float().contiguous().numpy()
  np.testing.assert_array_equal(value, _one_hot(labels.numpy()[:, None], C))
  cfg = dict(width=W, height=H, hfov=np.radians(70.), cam_pitch=np.radians(-20.),
             cam_height=0.88, width_offset=64., height_offset=64., map_res=0.06,
             map_width=128, map_height=128, trunc_depth_min=0.15, trunc_depth_max=5.05,
             to_global=True, fill_value=0.0)
  before = _one_hot_call(dmap, cfg, depth, value, cam_pose=pose)
  got, route = _label_call(dmap, cfg, depth, labels.numpy()[:, None], C, cam_pose=pose)
  after = _one_hot_call(dmap, cfg, depth, value, cam_pose=pose)
  assert route == NATIVE
  want = oracle.orth_project(depth, value_map=value, get_height_map=True,
                             **dict(project_kwargs(cfg, oracle.camera_intrinsics), cam_pose=pose))
  _assert_same(got, before, "label vs one-hot")
  _assert_same(got, (want[0], want[1], np.ascontiguousarray(want[2])), "label vs oracle")
  _assert_same(after, before, "one-hot call after the label call")
  assert got[1].any() and not got[1].all()


# ---- 3. the matrix ------------------------------------------------------------------------------
FILLS = [None, 0.0, 1.0, 0.5, 2.0, -np.inf, np.inf, np.nan]
DTYPES = [np.uint8, np.int16, np.int32, np.int64]
EXTRAS = ["valid", "clip", "notrunc", "pitch", "local", "noflip", "plain"]


def _matrix():
  cases, i = [], 0
  for red in ("max", "min"):                               # max and min against every fill, native route
    for fill in FILLS:
      classes = [1, 2, 31, 32, 33, 63, 5, 40][(i * 3) % 8]
      cases.append((red, fill, DTYPES[i % 4], EXTRAS[i % 7], [1, 3, 65][i % 3], [47, 48][i % 2], classes))
      i += 1
  for red in ("sum", "mean", "prod"):
    for fill in (FILLS[i % 8], FILLS[(i + 3) % 8], 0.0):
      cases.append((red, fill, DTYPES[i % 4], EXTRAS[i % 7], [1, 3, 65][i % 3], [47, 48][i % 2],
                    [5, 63, 64][i % 3]))
      i += 1
  # what the rotation above leaves out: the largest batch on the native route with the class limit,
  # the limit's neighbours on both reductions
  cases += [("max", np.nan, np.uint8, "plain", 3, 48, 64), ("min", np.inf, np.int16, "valid", 1, 47, 200),
            ("max", -np.inf, np.int32, "local", 65, 48, 200), ("min", None, np.int64, "clip", 3, 47, 64),
            ("max", 0.0, np.uint8, "plain", 65, 48, 63), ("min", -np.inf, np.int64, "valid", 65, 47, 63),
            ("min", 0.0, np.int32, "pitch", 3, 48, 64), ("max", None, np.int16, "clip", 3, 47, 33),
            ("min", 1.0, np.uint8, "notrunc", 1, 48, 32), ("max", 2.0, np.int64, "local", 3, 48, 31)]
  return cases


def test_matrix_covers_every_value_of_every_axis():
  cases = _matrix()
  assert {c[0] for c in cases} == {"max", "min", "sum", "mean", "prod"}
  for red in ("max", "min"):
    assert [repr(c[1]) for c in cases if c[0] == red][:8] == [repr(f) for f in FILLS]
  assert {c[2] for c in cases} == set(DTYPES) and {c[3] for c in cases} == set(EXTRAS)
  assert {c[4] for c in cases} == {1, 3, 65} and {c[5] for c in cases} == {47, 48}
  assert {c[6] for c in cases} >= {1, 2, 31, 32, 33, _limit(), _limit() + 1, 200}


@pytest.mark.parametrize("red,fill,dtype,extra,B,mw,C", _matrix())
def test_label_call_equals_one_hot_call(dmap, red, fill, dtype, extra, B, mw, C):
  H, W = 37, 51                                            # H * W is not a multiple of four
  depth, pose = _synthetic(B, H, W, seed=B * 100 + C)
  rng = np.random.default_rng(C * 7 + B)
  labels = rng.integers(0, C, size=(B, 1, H, W)).astype(dtype)        # (wraps for uint8 over 256 classes: fine)
  cfg = dict(width=W, height=H, hfov=np.radians(70.), cam_pitch=np.radians(-20.), cam_height=0.88,
             width_offset=mw / 2., height_offset=24., map_res=0.12, map_width=mw, map_height=48,
             trunc_depth_min=0.15, trunc_depth_max=5.05, to_global=True, fill_value=fill, reduction=red)
  valid = None
  if extra == "valid":
    valid = rng.random((B, 1, H, W)) < 0.7
  elif extra == "clip":
    cfg["clip_border"] = 3
  elif extra == "notrunc":
    cfg["trunc_depth_min"] = cfg["trunc_depth_max"] = None
  elif extra == "pitch":
    cfg["cam_pitch"] = np.linspace(-0.6, 0.3, B).astype(np.float32)
    cfg["trunc_height_max"] = 1.5
  elif extra == "local":
    cfg["to_global"] = False
  elif extra == "noflip":
    cfg["flip_h"] = False
  value = _one_hot(labels, C)
  got, route = _label_call(dmap, cfg, depth, labels, C, valid=valid, cam_pose=pose)
  want = _one_hot_call(dmap, cfg, depth, value, valid=valid, cam_pose=pose)
  assert route == (NATIVE if red in ("max", "min") and C <= _limit() else COMPAT)
  _assert_same(got, want, f"{red} fill={fill} {dtype.__name__} {extra} B={B} mw={mw} C={C}")
  assert got[0].shape == (B, C, 48, mw) and got[2].shape == (B, C, 48, mw)
  assert np.isfinite(got[2]).any()                         # the frames do reach their maps


# ---- 4. labels outside [0, num_classes) -----------------------------------------------------------
@pytest.mark.parametrize("red", ["max", "min", "mean"])
@pytest.mark.parametrize("dtype,voids", [(np.int64, (-1, 255, 7, 2 ** 40)), (np.int16, (-1, 255, 7)),
                                         (np.int32, (-2 ** 31, 7)), (np.uint8, (255, 7))])
def test_out_of_range_labels_are_points_of_no_class(dmap, red, dtype, voids):
  B, H, W, C = 2, 36, 52, 7
  depth, pose = _synthetic(B, H, W, seed=11)
  rng = np.random.default_rng(3)
  labels = rng.integers(0, C, size=(B, 1, H, W)).astype(dtype)
  pick = rng.integers(0, len(voids) * 2, size=labels.shape)
  for k, v in enumerate(voids):
    labels[pick == k] = v
  cfg = dict(width=W, height=H, hfov=np.radians(70.), cam_pitch=np.radians(-20.), cam_height=0.88,
             width_offset=24., height_offset=24., map_res=0.12, map_width=48, map_height=48,
             trunc_depth_min=0.15, trunc_depth_max=5.05, to_global=True, fill_value=-np.inf, reduction=red)
  value = _one_hot(labels, C)
  assert (value.sum(1) == 0).any() and (value.sum(1) == 1).any()
  got, route = _label_call(dmap, cfg, depth, labels, C, cam_pose=pose)
  assert route == (COMPAT if red == "mean" else NATIVE)
  _assert_same(got, _one_hot_call(dmap, cfg, depth, value, cam_pose=pose), f"{red} {dtype.__name__}")


@pytest.mark.parametrize("red,fill,cell,mask", [
    ("max", -np.inf, 0.0, True), ("max", 0.0, 0.0, False), ("max", 0.5, 0.5, False),
    ("min", np.inf, 0.0, True), ("min", -1.0, -1.0, False), ("min", 0.5, 0.0, True)])
def test_cells_hit_by_void_pixels_only(dmap, red, fill, cell, mask):
  """A hit cell without a class: max -> max(fill, 0), min -> min(fill, 0); mask = changed(out, fill)."""
  B, H, W, C = 1, 36, 52, 4
  depth, pose = _synthetic(B, H, W, seed=12)
  labels = np.full((B, 1, H, W), 255, np.uint8)
  cfg = dict(width=W, height=H, hfov=np.radians(70.), cam_pitch=np.radians(-20.), cam_height=0.88,
             width_offset=24., height_offset=24., map_res=0.12, map_width=48, map_height=48,
             trunc_depth_min=0.15, trunc_depth_max=5.05, to_global=True, fill_value=fill, reduction=red)
  (top, msk, height), route = _label_call(dmap, cfg, depth, labels, C, cam_pose=pose)
  assert route == NATIVE
  hit = np.isfinite(height)                                 # the height map marks the hit cells
  assert hit.any() and not hit.all() and hit.shape == top.shape
  np.testing.assert_array_equal(top[hit], np.full(hit.sum(), cell, np.float32))
  np.testing.assert_array_equal(top[~hit], np.full((~hit).sum(), fill, np.float32))
  np.testing.assert_array_equal(msk, hit & mask)


# ---- 5. routes ------------------------------------------------------------------------------------
def test_autograd_takes_the_compatibility_route(dmap):
  B, H, W, C = 2, 36, 52, 5
  depth, pose = _synthetic(B, H, W, seed=13)
  labels = np.random.default_rng(4).integers(0, C, size=(B, 1, H, W))
  cfg = dict(width=W, height=H, hfov=np.radians(70.), cam_pitch=np.radians(-20.), cam_height=0.88,
             width_offset=24., height_offset=24., map_res=0.12, map_width=48, map_height=48,
             trunc_depth_min=0.15, trunc_depth_max=5.05, to_global=True, fill_value=0.0)
  plain, route = _label_call(dmap, cfg, depth, labels, C, cam_pose=pose)
  assert route == NATIVE
  d = torch.from_numpy(depth).to(DEV).requires_grad_(True)
  proj = dmap.MapProjector(**cfg)
  top, mask, height = proj.orth_project(d, label_map=torch.from_numpy(labels).to(DEV), num_classes=C,
                                        cam_pose=pose, get_height_map=True)
  assert _route() == COMPAT
  assert height.requires_grad
  _assert_same(_np((top.detach(), mask, height.detach())), plain, "grad route")
  v = torch.from_numpy(_one_hot(labels, C)).to(DEV)
  d2 = torch.from_numpy(depth).to(DEV).requires_grad_(True)
  want = proj.orth_project(d2, value_map=v, cam_pose=pose, get_height_map=True)
  height.sum().backward()
  want[2].sum().backward()
  torch.cuda.synchronize()
  np.testing.assert_array_equal(d.grad.cpu().numpy(), d2.grad.cpu().numpy())
  assert (d.grad != 0).any()
  with torch.no_grad():                                    # grad mode off: the native route again
    proj.orth_project(d, label_map=torch.from_numpy(labels).to(DEV), num_classes=C, cam_pose=pose)
  assert _route() == NATIVE


# ---- 6. degenerate and plumbing ---------------------------------------------------------------------
def _small_cfg(**over):
  cfg = dict(width=52, height=36, hfov=np.radians(70.), cam_pitch=np.radians(-20.), cam_height=0.88,
             width_offset=24., height_offset=24., map_res=0.12, map_width=48, map_height=48,
             trunc_depth_min=0.15, trunc_depth_max=5.05, to_global=True, fill_value=0.0)
  cfg.update(over)
  return cfg


@pytest.mark.parametrize("fill", [0.0, -np.inf, None])
def test_all_pixels_truncated_away(dmap, fill):
  depth = np.full((2, 1, 36, 52), 100.0, np.float32)
  labels = np.ones((2, 1, 36, 52), np.int32)
  (top, mask, height), route = _label_call(dmap, _small_cfg(fill_value=fill), depth, labels, 3)
  assert route == NATIVE and not mask.any() and np.isneginf(height).all()
  np.testing.assert_array_equal(top, np.full(top.shape, 0.0 if fill is None else fill, np.float32))


def test_cpu_numpy_labels_in_cpu_tensors_out(dmap):
  depth, pose = _synthetic(1, 36, 52, seed=14)
  labels = np.random.default_rng(5).integers(0, 6, size=(36, 52, 1))          # int64, (h, w, 1)
  assert labels.dtype == np.int64
  proj = dmap.MapProjector(**_small_cfg())
  outs = proj.orth_project(depth[0], label_map=labels, num_classes=6, cam_pose=pose[0], get_height_map=True)
  assert _route() == NATIVE
  assert all(o.device.type == "cpu" for o in outs) and outs[1].dtype == torch.bool
  value = _one_hot(labels.reshape(1, 1, 36, 52), 6)
  want = proj.orth_project(depth[0], value_map=value[0], cam_pose=pose[0], get_height_map=True)
  _assert_same([o.numpy() for o in outs], [w.numpy() for w in want], "cpu round trip")
  # the same through device=: CPU inputs, outputs on the named device
  outs = proj.orth_project(depth[0], label_map=labels, num_classes=6, cam_pose=pose[0], device="cuda:0")
  assert outs[0].device.type == "cuda"
  np.testing.assert_array_equal(outs[0].cpu().numpy(), want[0].numpy())


def test_non_default_stream(dmap):
  depth, pose = _synthetic(3, 36, 52, seed=15)
  labels = np.random.default_rng(6).integers(0, 9, size=(3, 1, 36, 52)).astype(np.uint8)
  want, _ = _label_call(dmap, _small_cfg(), depth, labels, 9, cam_pose=pose)
  proj = dmap.MapProjector(**_small_cfg())
  d, l = torch.from_numpy(depth).to(DEV), torch.from_numpy(labels).to(DEV)
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    outs = proj.orth_project(d, label_map=l, num_classes=9, cam_pose=pose, get_height_map=True)
  side.synchronize()
  assert _route() == NATIVE
  _assert_same([o.cpu().numpy() for o in outs], want, "side stream")


def test_captured_in_a_graph_and_replayed(dmap):
  """Single-branch capture of the label call; replays project whatever the input buffers hold."""
  B, H, W, C = 2, 480, 640, 5
  cfg = dict(width=W, height=H, hfov=np.radians(70.), cam_pitch=np.radians(-20.), cam_height=0.88,
             width_offset=256., height_offset=256., map_res=0.03, map_width=512, map_height=512,
             trunc_depth_min=0.15, trunc_depth_max=5.05, to_global=True, fill_value=0.0)
  depth, pose = _synthetic(B, H, W, seed=16)
  rng = np.random.default_rng(7)
  labels = rng.integers(0, C, size=(B, 1, H, W)).astype(np.uint8)
  proj = dmap.MapProjector(**cfg)
  d, l = torch.from_numpy(depth).to(DEV), torch.from_numpy(labels).to(DEV)
  call = lambda: proj.orth_project(d, label_map=l, num_classes=C, cam_pose=pose, get_height_map=True)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(2):                      # warm-up outside the capture
      call()
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    outs = call()
  assert _route() == NATIVE
  for seed in (0, 1):
    if seed:                                # other inputs in the captured buffers
      d.copy_(torch.from_numpy(_synthetic(B, H, W, seed=17)[0]))
      l.copy_(torch.from_numpy(rng.integers(0, C, size=(B, 1, H, W)).astype(np.uint8)))
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in outs]
    want = call()
    torch.cuda.synchronize()
    for g_, w_ in zip(got, want):
      assert torch.equal(g_, w_)
    assert got[1].any()
