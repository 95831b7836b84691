"""An independent numpy restatement of what gets reduced into the cells (TEST INFRASTRUCTURE ONLY).

The reference's scatter_tensor (utils.py:389-492) fills the canvas (or keeps the caller's), keeps a
copy, hands both to torch_scatter's "reduce into `out`" and derives the mask from the difference.
This module states those rules once more, without the oracle's C reduction (dmo_reduce /
dmo_mask), so that the oracle, the HIP kernels and these rules are three separate statements:

* max / min: the points are visited in the reference's order (frame, pixel row-major) and a point is
  stored only if new > old (new < old for min).  A NaN value therefore never lands and a NaN cell
  never changes; among equal values the first one stays.
* sum: accumulated in float64, then added to the canvas.
* mean: (canvas + sum) / max(count, 1) -- the count includes every point that reached the cell,
  whatever its value (NaN and infinities included).
* prod: multiplied into the canvas in float32, one rounding per point, in the visiting order.
* mask: nan_to_num(|canvas - copy|, nan=0, posinf=1, neginf=1) != 0, so "inf - inf = NaN" and a
  NaN anywhere mean "unchanged".

For sum and mean the float64 accumulation equals the reference's float32 one whenever the float32
partial sums are exact (small integers, halves): the tests that compare bit for bit use such values.

The geometry (which pixel lands in which cell, its height) comes from the oracle's per-pixel debug
output, which tests/test_oracle_golden.py pins to the reference.
"""
import numpy as np

F32 = np.float32
REDUCTIONS = ("max", "min", "sum", "mean", "prod")


def _reduce(canvas, cells, values, reduction):
  """Reduce `values` (n,) float32 into `canvas` (M,) float32 at `cells` (n,) (in range, in the
  visiting order); returns the new canvas (float32)."""
  canvas = np.array(canvas, dtype=F32, copy=True)
  cells = np.asarray(cells, dtype=np.int64)
  values = np.asarray(values, dtype=F32)
  if reduction in ("max", "min"):
    # Python floats hold float32 values exactly and compare them as float32 would
    out = canvas.tolist()
    if reduction == "max":
      for k, v in zip(cells.tolist(), values.tolist()):
        if v > out[k]:
          out[k] = v
    else:
      for k, v in zip(cells.tolist(), values.tolist()):
        if v < out[k]:
          out[k] = v
    return np.asarray(out, dtype=F32)
  if reduction == "prod":
    with np.errstate(all="ignore"):
      np.multiply.at(canvas, cells, values)
    return canvas
  if reduction in ("sum", "mean"):
    acc = np.zeros(canvas.shape, dtype=np.float64)
    with np.errstate(all="ignore"):
      np.add.at(acc, cells, values.astype(np.float64))
      total = (canvas.astype(np.float64) + acc).astype(F32)
    if reduction == "sum":
      return total
    count = np.bincount(cells, minlength=canvas.shape[0]).astype(F32)
    with np.errstate(all="ignore"):
      return (total / np.maximum(count, F32(1.0))).astype(F32)
  raise ValueError(reduction)


def changed_mask(canvas, copy):
  """utils.py:489-491."""
  with np.errstate(all="ignore"):
    d = np.abs(np.asarray(canvas, dtype=F32) - np.asarray(copy, dtype=F32))
  return np.nan_to_num(d, nan=0.0, posinf=1.0, neginf=1.0) != 0


def scatter_ref(canvas, flat_index, values, fill, reduction):
  """utils.scatter_tensor on pre-ravelled indices.  canvas (..., C, M); flat_index (..., Ci, N)
  int64 with Ci in {1, C} (entries < 0 or >= M are dropped); values (..., C, N); fill None keeps
  the canvas.  Returns (canvas, mask), both (..., C, M)."""
  canvas = np.asarray(canvas, dtype=F32)
  values = np.asarray(values, dtype=F32)
  flat_index = np.asarray(flat_index, dtype=np.int64)
  M = canvas.shape[-1]
  start = canvas.copy() if fill is None else np.full(canvas.shape, F32(fill), dtype=F32)
  values = np.broadcast_to(values, canvas.shape[:-1] + values.shape[-1:])
  index = np.broadcast_to(flat_index, values.shape)
  out = start.reshape(-1, M).copy()
  for row, (idx, val) in enumerate(zip(index.reshape(-1, index.shape[-1]),
                                       values.reshape(-1, values.shape[-1]))):
    ok = (idx >= 0) & (idx < M)
    out[row] = _reduce(out[row], idx[ok], val[ok], reduction)
  out = out.reshape(canvas.shape)
  return out, changed_mask(out, start)


def project_ref(depth, kw, value=None, valid=None):
  """orth_project's maps (reference maps.py:127-351) for oracle-style keyword arguments `kw`
  (conftest.project_kwargs plus cam_pose): cells, validity and heights from
  oracle.orth_project(..., debug=True), the reduction and mask from the rules above.

  Returns dict(map (B, oc, mh, mw), mask, height (B, oc, mh, mw): the NINF / max height map of the
  same pixels as orth_project(get_height_map=True) returns it, for height-only calls the map)."""
  from oracle import oracle
  kw = dict(kw)
  reduction = kw.get("reduction") or "max"
  reduction = getattr(reduction, "value", reduction)
  fill = kw.get("fill_value")
  depth = np.asarray(depth, dtype=F32)
  if depth.ndim == 3:
    depth = depth[None]
  dbg = oracle.orth_project(depth, value_map=value, valid_map=valid, debug=True, **kw)[-1]
  B, dc, H, W = depth.shape
  mh, mw = int(kw["map_height"]), int(kw["map_width"])
  xb, zb, y = dbg["x_bin"], dbg["z_bin"], dbg["y"]
  ok = dbg["valid"] & (xb >= 0) & (xb < mw) & (zb >= 0) & (zb < mh)   # utils.py:455-461
  cells = np.where(ok, zb * mw + xb, -1)
  vals = None if value is None else np.asarray(value, dtype=F32).reshape(B, -1, H * W)
  vc = 0 if vals is None else vals.shape[1]
  oc = vc or dc
  start = np.full((mh * mw,), F32(0.0 if fill is None else fill), dtype=F32)
  out = np.empty((B, oc, mh * mw), dtype=F32)
  mask = np.empty((B, oc, mh * mw), dtype=bool)
  height = np.empty((B, dc, mh * mw), dtype=F32)
  for b in range(B):
    for ch in range(dc):
      sel = ok[b, ch]
      height[b, ch] = _reduce(np.full((mh * mw,), -np.inf, dtype=F32), cells[b, ch][sel],
                              y[b, ch][sel], "max")
    for k in range(oc):
      ch = k if dc > 1 else 0
      sel = ok[b, ch]
      src = y[b, ch] if not vc else vals[b, k]
      out[b, k] = _reduce(start, cells[b, ch][sel], src[sel], reduction)
      mask[b, k] = changed_mask(out[b, k], start)
  shape = (B, -1, mh, mw)
  out, mask, height = out.reshape(shape), mask.reshape(shape), height.reshape(shape)
  if vc and dc == 1:
    height = np.broadcast_to(height, out.shape)      # maps.py:349: one height map for every channel
  return dict(map=out, mask=mask, height=out if not vc else height)


# ------------------------------------------------------------------ inputs
FLT_MAX = np.finfo(F32).max
FLT_TRUE_MIN = np.float32(1e-45)          # the smallest denormal


def edge_values(rng, shape, reduction, rate=0.04):
  """Value maps of small integers {-2..2} (any summation order is exact) with NaN, +inf, -inf and
  -0.0 sprinkled in, and for max / min also +-FLT_MAX and +-the smallest denormal.  For prod the
  integers are mostly +-1 so that no cell's product overflows (an overflow would make 0 * inf
  order-dependent)."""
  if reduction == "prod":
    v = rng.choice(np.array([-1, 1, 1, -1, 2, -2, 0.5], dtype=F32), size=shape,
                   p=[0.4, 0.4, 0.05, 0.05, 0.04, 0.04, 0.02])
  else:
    v = rng.integers(-2, 3, size=shape).astype(F32)
  specials = [np.nan, np.inf, -np.inf, -0.0]
  if reduction in ("max", "min"):
    specials += [FLT_MAX, -FLT_MAX, FLT_TRUE_MIN, -FLT_TRUE_MIN]
  if reduction == "prod":
    specials += [0.0]
  flat = v.reshape(-1)
  at = rng.random(flat.size) < rate
  flat[at] = np.asarray(specials, dtype=F32)[rng.integers(0, len(specials), int(at.sum()))]
  return v


def scene_depth(rng, B, H, W):
  """Floor and wall depth (tests/campaigns/parity_campaign.py): many pixels per cell, tied heights."""
  rows = np.arange(H, dtype=np.float64).reshape(1, 1, H, 1)
  wall = rng.uniform(1.0, 6.0, size=(B, 1, 1, W // 8 + 1)).repeat(8, axis=3)[..., :W]
  floor = 0.9 / np.maximum(0.05, (rows - H * 0.45) / (H * 0.9))
  return np.broadcast_to(np.minimum(floor, wall).astype(F32), (B, 1, H, W)).copy()
