"""CPU checks of tests/scatter_semantics_ref.py: the independent statement of what gets reduced
into the cells agrees with the reference's own recorded results (g7) and with the oracle's C
reduction on value maps full of special values."""
import numpy as np
import pytest

from conftest import assert_masks_equal_away_from_fill, load_golden, project_kwargs
from scatter_semantics_ref import (FLT_MAX, REDUCTIONS, edge_values, project_ref, scatter_ref,
                                   scene_depth)

G7_CASES = (("min", np.inf), ("min", 0.0), ("sum", 0.0), ("sum", 1.0), ("mean", 0.0),
            ("mean", 2.0), ("prod", 1.0), ("max", 0.0), ("max", 1.0))


def _same_bits(got, want, what=""):
  got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
  assert got.shape == want.shape, what
  bad = got.view(np.uint32) != want.view(np.uint32)
  bad &= ~(np.isnan(got) & np.isnan(want))
  assert not bad.any(), f"{what}: {int(bad.sum())} cells differ, first {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.parametrize("red,fill", G7_CASES)
def test_project_ref_matches_g7(oracle, red, fill):
  """The reference's recorded maps, heights and values, with test_oracle_golden's bars."""
  g, cfg = load_golden("g7_reductions_64x48")
  kw = dict(project_kwargs(cfg, oracle.camera_intrinsics), reduction=red, fill_value=fill)
  tag = f"{red}_fill{fill}"
  for prefix, value in (("", g["value"]), ("height_", None)):
    got = project_ref(g["depth"], kw, value=value)
    want = g[f"{prefix}topdown_{tag}"]
    if red in ("max", "min"):
      _same_bits(got["map"], want, tag)
      np.testing.assert_array_equal(got["mask"], g[f"{prefix}mask_{tag}"])
    else:
      np.testing.assert_allclose(got["map"], want, rtol=1e-5, atol=1e-6)
      assert_masks_equal_away_from_fill(got["mask"], g[f"{prefix}mask_{tag}"], want, fill,
                                        exact=(prefix == ""), what=tag)


def _seeded_case(oracle, seed):
  rng = np.random.default_rng(9_100 + seed)
  B, H, W, mh, mw = 2, 24, 32, 24, 24
  red = REDUCTIONS[seed % 5]
  depth = scene_depth(rng, B, H, W) if seed % 3 else rng.uniform(0.1, 6.0, (B, 1, H, W)).astype(np.float32)
  integers = seed % 4 != 3                       # else normal reals (order-dependent sums)
  C = int(rng.choice([1, 2, 3]))
  dc = 1
  if seed % 7 == 2:                              # one value channel per depth channel
    dc = C
    depth = np.concatenate([depth * np.float32(1 + 0.1 * k) for k in range(dc)], axis=1)
  if integers:
    value = edge_values(rng, (B, C, H, W), red, rate=0.08)
  else:
    value = rng.normal(size=(B, C, H, W)).astype(np.float32)
    value.reshape(-1)[rng.integers(0, value.size, 20)] = np.resize(
        np.array([np.nan, np.inf, -np.inf, -0.0], np.float32), 20)
  fill = [None, 0.0, 1.5, -np.inf, np.inf, np.nan, -np.nan][seed % 7]
  valid = rng.uniform(size=(B, 1, H, W)) > 0.2 if seed % 2 else None
  pose = np.stack([rng.uniform(-0.3, 0.3, B), rng.uniform(-0.3, 0.3, B),
                   rng.uniform(-0.5, 0.5, B)], axis=1).astype(np.float32)
  cx, cy, fx, fy = oracle.camera_intrinsics(W, H, np.radians(70.))
  kw = dict(cam_pose=pose, width_offset=mw / 2., height_offset=2., cam_pitch=np.radians(-20.),
            cam_height=0.88, map_res=0.2, map_width=mw, map_height=mh, focal_x=fx, focal_y=fy,
            center_x=cx, center_y=cy, trunc_depth_min=0.15, trunc_depth_max=5.05,
            to_global=True, fill_value=fill, reduction=red)
  return depth, value, valid, kw, integers


@pytest.mark.parametrize("seed", range(10))
def test_project_ref_matches_oracle_on_special_values(oracle, seed):
  depth, value, valid, kw, integers = _seeded_case(oracle, seed)
  red = kw["reduction"]
  for v in (value, None):
    got = project_ref(depth, kw, value=v, valid=valid)
    want = oracle.orth_project(depth, value_map=v, valid_map=valid, get_height_map=True, **kw)
    what = f"seed {seed} {red} fill {kw['fill_value']} {'values' if v is not None else 'heights'}"
    assert got["mask"].any() or not np.isfinite(kw["fill_value"] or 0.0), what
    np.testing.assert_array_equal(np.isnan(got["map"]), np.isnan(want[0]), err_msg=what)
    np.testing.assert_array_equal(got["mask"], want[1], err_msg=what)
    if v is not None:                            # (height-only: the height map is the map)
      _same_bits(got["height"], np.ascontiguousarray(want[2]), what + " height")
    if red in ("max", "min") or (integers and v is not None):
      _same_bits(got["map"], want[0], what)
    else:
      inf = np.isinf(want[0])
      np.testing.assert_array_equal(got["map"][inf], want[0][inf], err_msg=what)
      np.testing.assert_allclose(got["map"], want[0], rtol=1e-5, atol=1e-6, err_msg=what)


def test_scatter_ref_rules():
  """Hand-worked cells: the rules the kernels' special cases encode."""
  nan, inf = np.float32(np.nan), np.float32(np.inf)
  canvas = np.array([[[0.0, nan, -nan, inf, -inf, 1.0, 2.0, 3.0]]], np.float32)
  idx = np.array([[[0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5, 7, 7, 7, -1, 8]]])
  vals = np.array([[[nan, 5.0, 5.0, 1.0, 1.0, 2.0, -5.0, -5.0, inf, -inf, nan, 1.0, nan, 4.0,
                     9.0, 9.0]]], np.float32)
  out, mask = scatter_ref(canvas, idx, vals, None, "max")
  _same_bits(out, [[[2.0, nan, nan, inf, 1.0, 1.0, 2.0, 4.0]]])
  np.testing.assert_array_equal(mask, [[[1, 0, 0, 0, 1, 0, 0, 1]]])
  out, mask = scatter_ref(canvas, idx, vals, None, "sum")
  _same_bits(out, [[[nan, nan, nan, inf, -inf, nan, 2.0, nan]]])
  np.testing.assert_array_equal(mask, 0)
  out, mask = scatter_ref(canvas, idx, vals, 1.5, "mean")
  _same_bits(out, [[[nan, 0.75, 0.75, inf, -inf, nan, 1.5, nan]]])
  np.testing.assert_array_equal(mask, [[[0, 1, 1, 1, 1, 0, 0, 0]]])
  out, mask = scatter_ref(canvas, idx, vals, None, "prod")
  _same_bits(out, [[[nan, nan, nan, inf, inf, nan, 2.0, nan]]])
  np.testing.assert_array_equal(mask, [[[0, 0, 0, 0, 1, 0, 0, 0]]])
  out, mask = scatter_ref(np.zeros((1, 1, 2), np.float32), np.array([[[0, 0, 1]]]),
                          np.array([[[FLT_MAX, FLT_MAX, -FLT_MAX]]], np.float32), None, "sum")
  _same_bits(out, [[[inf, -FLT_MAX]]])
  np.testing.assert_array_equal(mask, [[[1, 1]]])
