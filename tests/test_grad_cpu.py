"""orth_project's backward without a GPU: argument checks of the two native entry points, and the
numpy expected-gradient helper (tests/grad_expect.py, fed by the CPU oracle) against the
reference's own gradients (g14, tests/golden/gen_golden_grad.py).

Bar: value gradients bit-exact, depth / camera gradients within 1e-5 relative."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from grad_expect import expected_grads


def _params(**kw):
  from dungeon_maps_amd import _native
  p = _native.Params()
  p.B, p.dc, p.vc, p.H, p.W, p.mh, p.mw = 1, 1, 0, 8, 8, 8, 8
  p.reduction = _native.REDUCE_MAX
  p.fx = p.fy = 4.0
  p.res = 0.1
  for k, v in kw.items():
    setattr(p, k, v)
  return p


def _winners(p, frames=1, depth=1, value=None, out=1, height=None, win=1, hwin=None, ws=1, ws_bytes=4096):
  from dungeon_maps_amd import _native
  return _native.lib().dm_orth_project_winners_f32(ctypes.byref(p), frames, depth, value, None, out,
                                                   height, win, hwin, ws, ws_bytes, None)


def _backward(p, frames=1, depth=1, win=1, hwin=None, gout=1, gh=None, gval=None, gdep=1, mom=None,
              ws=1, ws_bytes=4096):
  from dungeon_maps_amd import _native
  return _native.lib().dm_orth_project_backward_f32(ctypes.byref(p), frames, depth, None, win, hwin, gout,
                                                    gh, gval, gdep, mom, ws, ws_bytes, None)


def test_backward_entry_points_refuse_bad_arguments_before_any_hip_call():
  # (the pointers are never dereferenced: every call below is refused up front)
  from dungeon_maps_amd import _native
  lib = _native.lib()
  assert lib.dm_version() == 11
  err = lambda: lib.dm_last_error().decode()
  assert _winners(_params(reduction=_native.REDUCE_PROD)) == -2 and "prod" in err()
  assert _backward(_params(reduction=_native.REDUCE_PROD)) == -2 and "prod" in err()
  assert _winners(_params(reduction=9)) == -1 and "reduction" in err()
  assert _backward(_params(dc=0)) == -1 and "shape" in err()
  assert _winners(_params(vc=3, dc=2), value=1) == -1 and "channels" in err()
  assert _winners(_params(), ws_bytes=8) == -3
  assert _backward(_params(B=4), ws_bytes=128) == -3
  assert _winners(_params(reduction=_native.REDUCE_SUM)) == -1 and "sum" in err()
  assert _winners(_params(), hwin=1) == -1 and "height" in err()
  assert _winners(_params(vc=2), value=None) == -1 and "value" in err()
  assert _backward(_params(), win=None) == -1 and "winners" in err()
  assert _backward(_params(), gval=1) == -1 and "value map" in err()
  assert _backward(_params(vc=2), gh=1, hwin=None) == -1 and "height winners" in err()
  assert _backward(_params(), frames=None) == -1
  assert "dm_orth_project_winners_f32" in _native.exported_symbols()
  assert "dm_orth_project_backward_f32" in _native.exported_symbols()


def _cases():
  arrays, cfg = load_golden("g14_orth_project_grad")
  return arrays, cfg, [str(c) for c in arrays["cases"]]


_ARR, _CFG, _NAMES = _cases()


def case_config(name):
  """(arrays of one g14 case, orth_project keyword arguments of it)."""
  a = {k.split("/", 1)[1]: v for k, v in _ARR.items() if k.startswith(name + "/")}
  c = {k[4:]: (v.item() if v.ndim == 0 else v) for k, v in a.items() if k.startswith("cfg_")}
  nan = lambda v: None if isinstance(v, float) and np.isnan(v) else v
  from oracle import oracle
  cx, cy, fx, fy = oracle.camera_intrinsics(_CFG["width"], _CFG["height"], _CFG["hfov"])
  kw = dict(cam_pose=a["cam_pose"], width_offset=_CFG["width_offset"], height_offset=_CFG["height_offset"],
            cam_pitch=a["pitch"], cam_height=a["cam_height"], map_res=_CFG["map_res"],
            map_width=_CFG["map_width"], map_height=_CFG["map_height"], focal_x=fx, focal_y=fy,
            center_x=cx, center_y=cy, trunc_depth_min=nan(c["dmin"]), trunc_depth_max=nan(c["dmax"]),
            trunc_height_max=nan(c["hmax"]), clip_border=c["clip"] or None, to_global=bool(c["to_global"]),
            flip_h=bool(c["flip_h"]), fill_value=None if c["fill_is_none"] else c["fill"],
            reduction=c["reduction"], get_height_map=bool(c["get_height"]))
  return a, kw


def helper_grads(a, kw, topdown, mask):
  """expected_grads for one g14 case, fed the oracle's intermediates."""
  from oracle import oracle
  okw = {k: v for k, v in kw.items() if k != "get_height_map"}
  res = oracle.orth_project(a["depth"], value_map=a.get("value"), valid_map=a.get("valid"),
                            debug=True, **okw)
  dbg = res[-1]
  return expected_grads(dbg, a["depth"], topdown, mask, W_top=a["weights"], W_height=a.get("hweights"),
                        value=a.get("value"), reduction=kw["reduction"], pitch=kw["cam_pitch"],
                        H=a["depth"].shape[2], W=a["depth"].shape[3], cx=kw["center_x"], cy=kw["center_y"],
                        fx=kw["focal_x"], fy=kw["focal_y"], flip_h=kw["flip_h"], mh=kw["map_height"],
                        mw=kw["map_width"])


def assert_close_rel(got, want, rtol=1e-5, what=""):
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  scale = max(np.abs(want).max(), 1e-30)
  err = np.abs(got - want).max() if got.size else 0.0
  assert err <= rtol * scale, f"{what}: max error {err:.3g} > {rtol:g} x {scale:.3g}"


@pytest.mark.parametrize("name", _NAMES)
def test_expected_gradient_helper_matches_reference_g14(name):
  a, kw = case_config(name)
  g_depth, g_value, g_pitch, g_h = helper_grads(a, kw, a["topdown"], a["mask"])
  if "grad_value" in a:
    np.testing.assert_array_equal(g_value, a["grad_value"])
  assert_close_rel(g_depth, a["grad_depth"], what="depth")
  assert_close_rel(g_pitch, a["grad_pitch"], what="pitch")
  assert_close_rel(g_h, a["grad_cam_height"], what="cam_height")
  if name == "max_pitch_clamp":
    assert a["grad_pitch"][0] == 0 and g_pitch[0] == 0
