"""What gets reduced into the cells, on every projection route and entry point and in the scatter
primitive, against the independent statement of the reference's rules (scatter_semantics_ref).

Value maps are small integers {-2..2} with NaN, +-inf and -0.0 sprinkled in (max / min also get
+-FLT_MAX and +-the smallest denormal), projected with the scene-like floor / wall depth so that many
pixels share a cell.  Every summation order of such values is exact, so sum / mean / prod maps are
compared bit for bit too.  The bars:

* maps equal the reference's bit for bit, except that -0.0 and +0.0 count as equal: the reference's
  winner among +-0 depends on the order in which the points arrive, so the sign of a zero is not
  pinned;
* NaN positions and masks equal the reference's exactly;
* since every route is held to the same reference under the same bar, every route equals every
  other route;
* a batch-fused map equals amax / amin over the frames of the reference's per-frame maps.

Where an entry point refuses a (reduction, fill) pair it must raise its documented error.
"""
import ctypes

import numpy as np
import pytest
import torch

from scatter_semantics_ref import (REDUCTIONS, changed_mask, edge_values, project_ref, scatter_ref,
                                   scene_depth)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FILLS = (None, 0.0, 1.5, -np.inf, np.inf, NAN, -NAN)


@pytest.fixture(scope="module")
def dmap():
  import dungeon_maps_amd as dmap
  from dungeon_maps_amd import _native
  _native.lib()
  if not torch.cuda.is_available():
    pytest.fail("GPU tests need cuda:0")
  return dmap


def _fid(f):
  return "None" if f is None else ("-nan" if np.isnan(f) and np.signbit(f) else str(f))


def _is_nan(f):
  return f is not None and np.isnan(f)


def _same(got, want, what):
  """Bit for bit with +0 == -0; NaN exactly where the reference has NaN."""
  got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
  want = np.asarray(want)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  gn, wn = np.isnan(got), np.isnan(want)
  bad = (gn != wn) | (~gn & ~wn & (got != want))
  if bad.any():
    at = tuple(np.argwhere(bad)[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} cells differ, first at {at}: "
                         f"got {got[at]!r} want {want[at]!r}")


def _same_mask(got, want, what):
  got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
  bad = got != np.asarray(want)
  if bad.any():
    at = tuple(np.argwhere(bad)[0])
    raise AssertionError(f"{what}: {int(bad.sum())} mask cells differ, first at {at}: got {got[at]}")


def _geometry(oracle, B=2, H=48, W=64, mh=64, mw=64, res=0.1, dc=1, seed=0):
  rng = np.random.default_rng(777 + seed)
  depth = scene_depth(rng, B, H, W)
  if dc > 1:
    depth = np.concatenate([depth * np.float32(1 + 0.1 * k) for k in range(dc)], axis=1)
  cx, cy, fx, fy = oracle.camera_intrinsics(W, H, np.radians(70.))
  pose = np.array([[0.1, 0.05, 0.2], [-0.1, 0.1, -0.3], [0.0, -0.1, 0.1]][:B], np.float32)
  kw = dict(cam_pose=pose, width_offset=mw / 2., height_offset=mh / 2., cam_pitch=np.radians(-20.),
            cam_height=0.88, map_res=res, map_width=mw, map_height=mh, focal_x=fx, focal_y=fy,
            center_x=cx, center_y=cy, trunc_depth_min=0.15, trunc_depth_max=5.05,
            trunc_height_max=None, clip_border=None, to_global=True)
  return depth, kw


def _values(red, shape, seed=0):
  return edge_values(np.random.default_rng(31 + 7 * REDUCTIONS.index(red) + seed), shape, red)


def _gpu(a):
  return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Route:
  """A projection route forced with the library's test hooks; `path` is what
  dm_debug_last_path reported for the last call inside it."""

  def __init__(self, name, legacy=0, bands=0, strips=0, generic=0):
    self.name, self.legacy, self.bands, self.strips, self.generic = name, legacy, bands, strips, generic
    self.path, self.split = None, None

  def __enter__(self):
    from dungeon_maps_amd import _native
    lib = _native.lib()
    lib.dm_debug_force_legacy_window(self.legacy)
    lib.dm_debug_force_bands(self.bands)
    lib.dm_debug_force_strips(self.strips)
    lib.dm_debug_force_generic_path(self.generic)
    return self

  def note(self):
    from dungeon_maps_amd import _native
    lib = _native.lib()
    self.path = lib.dm_debug_last_path()
    split = (ctypes.c_int32 * 4)()
    lib.dm_debug_last_split(split)
    self.split = list(split)

  def __exit__(self, *exc):
    from dungeon_maps_amd import _native
    lib = _native.lib()
    lib.dm_debug_force_legacy_window(0)
    lib.dm_debug_force_bands(0)
    lib.dm_debug_force_strips(0)
    lib.dm_debug_force_generic_path(0)


def _window_ok(red, fill, mw):
  """window_path_supported (dm_window.hip)."""
  return red != "prod" and not _is_nan(fill) and mw % 4 == 0


def _strips_ok(red, fill, mw, W):
  """make_plan (dm_strip.hip): max / min, a fill with an order, aligned widths, bounded depth."""
  return red in ("max", "min") and not _is_nan(fill) and mw % 4 == 0 and W % 4 == 0


def _routes(red, fill, mw, W):
  """(route, the path it must report or None).  Strips run for max / min only.  (A route the
  library refuses, and the generic route, leave dm_debug_last_path as it was: not checked.)"""
  out = [(_Route("default"), None),
         (_Route("window", legacy=1), 1 if _window_ok(red, fill, mw) else None),
         (_Route("generic", generic=1), None)]
  if red in ("max", "min"):
    out += [(_Route(f"strips{k}", strips=k), 2 if _strips_ok(red, fill, mw, W) else None)
            for k in range(1, 9)]
  return out


def _project(dmap, depth, kw, value, red, fill, get_height_map=True):
  return dmap.functional.orth_project(
      _gpu(depth), _gpu(value), None, fill_value=fill, reduction=red, get_height_map=get_height_map,
      **kw)


def _check_maps(got, want, what, height=True):
  _same(got[0], want["map"], what + " map")
  _same_mask(got[1], want["mask"], what + " mask")
  if height and len(got) > 2:
    _same(got[2], want["height"], what + " height")


@pytest.mark.parametrize("fill", FILLS, ids=_fid)
@pytest.mark.parametrize("red", REDUCTIONS)
def test_value_maps_on_every_route(dmap, oracle, red, fill):
  """orth_project(get_height_map=True) of a three-channel value map on the default route, the
  LDS-window route, the generic route and (max / min) the strip route at 1..8 strips."""
  depth, kw = _geometry(oracle)
  B, _, H, W = depth.shape
  value = _values(red, (B, 3, H, W))
  want = project_ref(depth, dict(kw, reduction=red, fill_value=fill), value=value)
  assert want["mask"].any() or _is_nan(fill) or (fill is not None and np.isinf(fill)) or \
      (red == "prod" and not fill)
  for route, path in _routes(red, fill, kw["map_width"], W):
    with route:
      got = _project(dmap, depth, kw, value, red, fill)
      route.note()
    torch.cuda.synchronize()
    what = f"{red} fill {_fid(fill)} route {route.name} (path {route.path})"
    if path is not None:
      assert route.path == path, what
    _check_maps(got, want, what)


@pytest.mark.parametrize("fill", (-np.inf, np.inf, NAN, -NAN), ids=_fid)
@pytest.mark.parametrize("red", REDUCTIONS)
def test_height_maps_on_every_route(dmap, oracle, red, fill):
  """Height-only projections with fills an infinity or NaN (every reduction is then exact: the fill
  dominates what the heights add), through orth_project, orth_project_and_flow and, for max / min,
  orth_project_fused."""
  depth, kw = _geometry(oracle)
  W = depth.shape[3]
  want = project_ref(depth, dict(kw, reduction=red, fill_value=fill))
  for route, path in _routes(red, fill, kw["map_width"], W):
    with route:
      got = _project(dmap, depth, kw, None, red, fill)
      route.note()
      flow = dmap.functional.orth_project_and_flow(
          _gpu(depth), np.array([0.05, 0.1, 0.02], np.float32), None, fill_value=fill, reduction=red,
          **kw)
    torch.cuda.synchronize()
    what = f"heights {red} fill {_fid(fill)} route {route.name} (path {route.path})"
    if path is not None:
      assert route.path == path, what
    _check_maps(got, want, what)
    assert got[2] is got[0]
    _check_maps(flow[:2], want, what + " orth_project_and_flow")
  _check_fused_entry(dmap, depth, kw, None, red, fill, want)


def _fused_ref(want, red, fill):
  maps = torch.from_numpy(want["map"])
  fused = (torch.amax if red == "max" else torch.amin)(maps, dim=0).numpy()
  start = np.full(fused.shape, np.float32(0.0 if fill is None else fill), np.float32)
  return fused, changed_mask(fused, start)


def _check_fused_entry(dmap, depth, kw, value, red, fill, want):
  """orth_project_fused: the batch in ONE map (max / min), else its documented refusal."""
  from dungeon_maps_amd._native import NativeError
  if red not in ("max", "min"):
    with pytest.raises(NativeError, match="supports max/min only"):
      dmap.functional.orth_project_fused(_gpu(depth), _gpu(value), None, fill_value=fill,
                                         reduction=red, **kw)
    return
  fmap, fmask = _fused_ref(want, red, fill)
  got = dmap.functional.orth_project_fused(_gpu(depth), _gpu(value), None, fill_value=fill,
                                           reduction=red, **kw)
  _same(got[0], fmap, f"orth_project_fused {red} fill {_fid(fill)}")
  _same_mask(got[1], fmask, f"orth_project_fused {red} fill {_fid(fill)} mask")


@pytest.mark.parametrize("fill", FILLS, ids=_fid)
@pytest.mark.parametrize("red", REDUCTIONS)
def test_value_maps_through_every_entry_point(dmap, oracle, red, fill):
  """orth_project_and_fuse (per-frame and fused maps), orth_project_fused and PreparedProjection
  where they accept the pair; their documented errors where they do not."""
  from dungeon_maps_amd._native import NativeError
  depth, kw = _geometry(oracle)
  B, _, H, W = depth.shape
  value = _values(red, (B, 3, H, W))
  want = project_ref(depth, dict(kw, reduction=red, fill_value=fill), value=value)
  what = f"{red} fill {_fid(fill)}"
  F = dmap.functional
  if red in ("max", "min"):
    top, mask, fused, fmask = F.orth_project_and_fuse(_gpu(depth), _gpu(value), None, fill_value=fill,
                                                      reduction=red, **kw)
    _check_maps((top, mask), want, what + " orth_project_and_fuse")
    fmap, fm = _fused_ref(want, red, fill)
    _same(fused, fmap, what + " orth_project_and_fuse fused")
    _same_mask(fmask, fm, what + " orth_project_and_fuse fused mask")
  else:
    with pytest.raises(NativeError, match="supports max/min only"):
      F.orth_project_and_fuse(_gpu(depth), _gpu(value), None, fill_value=fill, reduction=red, **kw)
  _check_fused_entry(dmap, depth, kw, value, red, fill, want)
  camera = {k: kw[k] for k in kw if k != "cam_pose"}
  if _strips_ok(red, fill, kw["map_width"], W):
    prep = F.prepare_orth_project(B, H, W, kw["cam_pose"], fill_value=fill, reduction=red,
                                  value_channels=3, **{k: v for k, v in camera.items()})
    got = prep.orth_project(_gpu(depth), _gpu(value), get_height_map=True)
    _check_maps(got, want, what + " PreparedProjection.orth_project")
    top, mask, fused, fmask = prep.orth_project_and_fuse(_gpu(depth), _gpu(value))
    _check_maps((top, mask), want, what + " PreparedProjection.orth_project_and_fuse")
    fmap, fm = _fused_ref(want, red, fill)
    _same(fused, fmap, what + " PreparedProjection fused")
    _same_mask(fmask, fm, what + " PreparedProjection fused mask")
  else:
    with pytest.raises(NativeError, match="cannot be prepared"):
      F.prepare_orth_project(B, H, W, kw["cam_pose"], fill_value=fill, reduction=red,
                             value_channels=3, **camera)


@pytest.mark.parametrize("fill", (None, 1.5, -np.inf, np.inf), ids=_fid)
@pytest.mark.parametrize("red", ("max", "min", "sum", "mean"))
def test_depth_bands_route(dmap, oracle, red, fill):
  """The LDS-window route with depth bands (dm_debug_force_bands) on a fine map."""
  depth, kw = _geometry(oracle, B=2, H=120, W=160, mh=512, mw=512, res=0.0125, seed=1)
  B, _, H, W = depth.shape
  value = _values(red, (B, 2, H, W), seed=1)
  want = project_ref(depth, dict(kw, reduction=red, fill_value=fill), value=value)
  route = _Route("bands", legacy=1, bands=1)
  with route:
    got = _project(dmap, depth, kw, value, red, fill)
    route.note()
  torch.cuda.synchronize()
  what = f"bands {red} fill {_fid(fill)} (path {route.path}, split {route.split})"
  assert route.path == 1 and route.split[2] > 1, what
  _check_maps(got, want, what)


@pytest.mark.parametrize("fill", FILLS, ids=_fid)
@pytest.mark.parametrize("red", REDUCTIONS)
def test_odd_width_and_per_channel_depth(dmap, oracle, red, fill):
  """A map width that is not a multiple of 4 (the padded route) and three depth channels with
  one value channel each (dc = vc = 3), on the default and the generic route."""
  for geo, C in ((dict(mw=63), 3), (dict(dc=3), 3)):
    depth, kw = _geometry(oracle, **geo)
    B, _, H, W = depth.shape
    value = _values(red, (B, C, H, W), seed=2)
    want = project_ref(depth, dict(kw, reduction=red, fill_value=fill), value=value)
    routes = [_Route("default"), _Route("generic", generic=1)]
    if red in ("max", "min") and geo.get("dc"):
      routes.append(_Route("strips2", strips=2))
    for route in routes:
      with route:
        got = _project(dmap, depth, kw, value, red, fill)
        route.note()
      torch.cuda.synchronize()
      _check_maps(got, want, f"{geo} {red} fill {_fid(fill)} route {route.name} (path {route.path})")


# ------------------------------------------------------------------ the scatter primitive
def _scatter_case(rng, red, shape, N, M):
  values = edge_values(rng, shape + (N,), red)
  canvas = edge_values(rng, shape + (M,), red, rate=0.2)
  canvas.reshape(-1)[:2] = [NAN, -NAN]            # a NaN cell with its sign bit set
  return values, canvas


@pytest.mark.parametrize("red", REDUCTIONS)
def test_scatter_tensor_special_values(dmap, red):
  """utils.scatter_tensor: special values in the values and in an existing canvas (including a NaN
  cell with its sign bit set), every fill, indices shared by all channels (Ci = 1) and given per
  channel (Ci = C), a 3-D batch shape, out-of-range and dropped points."""
  rng = np.random.default_rng(5 + REDUCTIONS.index(red))
  R, C, N, M = 2, 3, 700, 37
  values, canvas = _scatter_case(rng, red, (R, C), N, M)
  for Ci in (1, C):
    index = rng.integers(-3, M + 3, size=(R, Ci, N))
    for fill in FILLS:
      want, wmask = scatter_ref(canvas, index, values, fill, red)
      out, mask = dmap.utils.scatter_tensor(
          _gpu(canvas), _gpu(np.broadcast_to(index, (R, C, N))[..., None]), _gpu(values),
          fill_value=fill, reduction=red)
      what = f"scatter_tensor {red} Ci={Ci} fill {_fid(fill)}"
      _same(out, want, what)
      _same_mask(mask, wmask, what)
    # shared index rows straight into the flat primitive (Ci = 1 kept, not expanded)
    if Ci == 1:
      from dungeon_maps_amd import functional as F
      for fill in (None, 1.5):
        want, wmask = scatter_ref(canvas, index, values, fill, red)
        out, mask = F._scatter_flat(_gpu(canvas), _gpu(np.where((index >= 0) & (index < M), index, -1)),
                                    _gpu(values), 1, fill, red)
        _same(out, want, f"flat Ci=1 {red} fill {_fid(fill)}")
        _same_mask(mask, wmask, f"flat Ci=1 {red} fill {_fid(fill)} mask")
  # a 3-D batch shape (2, 2, 3) of 1-D canvases
  v3 = edge_values(rng, (2, 2, 3, 90), red)
  c3 = edge_values(rng, (2, 2, 3, 11), red, rate=0.3)
  i3 = rng.integers(-1, 12, size=(2, 2, 3, 90))
  for fill in (None, 0.0, -np.inf):
    want, wmask = scatter_ref(c3, i3, v3, fill, red)
    out, mask = dmap.utils.scatter_tensor(_gpu(c3), _gpu(i3[..., None]), _gpu(v3), fill_value=fill,
                                          reduction=red)
    _same(out, want, f"3-D batch {red} fill {_fid(fill)}")
    _same_mask(mask, wmask, f"3-D batch {red} fill {_fid(fill)} mask")


@pytest.mark.parametrize("red", REDUCTIONS)
def test_project_special_values_and_empty_input(dmap, red):
  """project(): (row, col) coordinates with a point mask; mean with a non-zero fill and with an
  existing canvas, prod without a fill; N = 0; every point masked or out of bounds."""
  rng = np.random.default_rng(50 + REDUCTIONS.index(red))
  b, c, n, mh, mw = 2, 3, 600, 6, 7
  coords = np.stack([rng.integers(-1, mh + 1, size=(b, 1, n)),
                     rng.integers(-1, mw + 1, size=(b, 1, n))], axis=-1)
  values = edge_values(rng, (b, c, n), red)
  masks = rng.uniform(size=(b, 1, n)) > 0.2
  canvas = edge_values(rng, (b, c, mh, mw), red, rate=0.2)
  canvas.reshape(-1)[:2] = [NAN, -NAN]
  inside = masks & (coords[..., 0] >= 0) & (coords[..., 0] < mh) & (coords[..., 1] >= 0) & \
      (coords[..., 1] < mw)
  flat = np.where(inside, coords[..., 0] * mw + coords[..., 1], -1)
  for fill in (None, 2.5, -np.inf, NAN):
    want, wmask = scatter_ref(canvas.reshape(b, c, -1), flat, values, fill, red)
    out, mask = dmap.project(_gpu(coords), _gpu(values), _gpu(masks), _gpu(canvas), fill_value=fill,
                             reduction=red)
    what = f"project {red} fill {_fid(fill)}"
    _same(out, want.reshape(b, c, mh, mw), what)
    _same_mask(mask, wmask.reshape(b, c, mh, mw), what)
  for name, m, co in (("N = 0", masks[..., :0], coords[:, :, :0]),
                      ("all masked", np.zeros_like(masks), coords),
                      ("all out of bounds", masks, coords + np.array([mh + 1, 0]))):
    for fill in (None, 1.5):
      out, mask = dmap.project(_gpu(co), _gpu(values[..., :co.shape[2]]), _gpu(m), _gpu(canvas),
                               fill_value=fill, reduction=red)
      want = canvas if fill is None else np.full_like(canvas, fill)
      _same(out, want, f"project {red} {name} fill {_fid(fill)}")
      assert not mask.any(), f"project {red} {name} fill {_fid(fill)}: mask set"


@pytest.mark.parametrize("red", REDUCTIONS)
def test_scatter_contention_one_cell(dmap, red):
  """10^5 points of +-1 into one cell (and a few into a second): exact answers for every
  reduction, the CAS multiply and the atomics under full contention."""
  rng = np.random.default_rng(9)
  N = 100_000
  values = rng.choice(np.array([-1.0, 1.0], np.float32), size=(1, 2, N))
  index = np.zeros((1, 1, N), np.int64)
  index[0, 0, :5] = 1
  canvas = np.zeros((1, 2, 3), np.float32)
  for fill in (None, 1.0):
    want, wmask = scatter_ref(canvas, index, values, fill, red)
    out, mask = dmap.utils.scatter_tensor(_gpu(canvas), _gpu(np.broadcast_to(index, (1, 2, N))[..., None]),
                                          _gpu(values), fill_value=fill, reduction=red)
    what = f"contention {red} fill {_fid(fill)}"
    _same(out, want, what)
    _same_mask(mask, wmask, what)
